"""The SAM texts of tests/test_sam_text_cpu.py and tests/test_gpu_sam.py -- TEST INFRASTRUCTURE ONLY.

cases() -> [(name, text bytes, refusal)]: refusal is None for a text the library takes, else (code name, 1-based line,
field, a string its message must hold or None).  The shapes are the smallest at which each kernel can go wrong: field
lengths on and next to the 64-byte step of the wave loops, the ends of every number range, and record counts on and
next to the sort's tile of 256 keys.
"""
from __future__ import annotations

import random

REFS = [("chr1", 100000), ("chr1b", 5000), ("chr10", 2 ** 31 - 1), ("a" * 200, 700), ("chrM", 16569), ("x|y:z", 99),
        ("chrU", 12345)]
HEADER = ("@HD\tVN:1.6\tGO:query\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
          + "@PG\tID:minimap2\tPN:minimap2\tVN:2.24\tCL:minimap2 -ax map-ont --cs ref.fa reads.fq\n")


def line(qname="r", flag=0, rname="chr1", pos=1, mapq=60, cigar=None, rnext="*", pnext=0, tlen=0, seq="ACGT", qual=None,
         aux=()):
    if cigar is None:
        cigar = "*" if seq == "*" else "%dM" % len(seq)
    if qual is None:
        qual = "*" if seq == "*" else "".join(chr(33 + (7 * k) % 60) for k in range(len(seq)))
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual,
                      *aux]) + "\n"


def _bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choices(alphabet, k=n))


def order_text(n, seed=5):
    """n records whose positions come from 50 values on 7 references, so that equal keys cross every tile and workgroup
    boundary of the sort: both strands at one position, POS 0 with a reference, flag 4 with a reference (placed by it)
    and records without one (last, in input order); primary records carry NM, cs and de as minimap2 writes them."""
    rng = random.Random(seed)
    spots = [0] + rng.sample(range(1, 5000), 49)
    out = []
    for i in range(n):
        u = rng.random()
        flag = 16 * (rng.random() < 0.5)
        rname, pos = rng.choice(REFS)[0], rng.choice(spots)
        if u < 0.06:
            flag, rname, pos = flag | 4, "*", 0
        elif u < 0.12:
            flag |= 4
        elif u < 0.2:
            flag |= rng.choice([256, 2048])
        k = rng.randint(1, 40)
        cs = ":%d" % k if rng.random() < 0.7 else ":%d*ag:%d" % (k // 2, k - k // 2)
        aux = ("NM:i:%d" % rng.randint(0, 3), "cs:Z:" + cs, "de:f:%.4f" % (rng.random() / 10)) if not flag & 4 else ()
        out.append(line("q%d" % i, flag, rname, pos, rng.randint(0, 60), seq=_bases(rng, k), aux=aux))
    return HEADER + "".join(out)


def cases():
    rng = random.Random(20)
    C = []

    def ok(name, text):
        C.append((name, text.encode("latin-1"), None))

    def no(name, text, code, lineno, field, holds=None):
        C.append((name, text.encode("latin-1"), (code, lineno, field, holds)))

    nh = HEADER.count("\n")
    # ---- lines
    ok("no_record_at_all", "")
    ok("header_only", HEADER)
    ok("header_without_final_newline", HEADER[:-1])
    ok("one_record", HEADER + line())
    ok("last_line_without_newline", HEADER + line("a") + line("b", pos=9)[:-1])
    ok("no_header_line_hd", HEADER.split("\n", 1)[1] + line())
    ok("hd_without_so", "@HD\tVN:1.5\n" + HEADER.split("\n", 1)[1] + line())
    ok("records_without_any_header", line(rname="*", pos=0, flag=4))
    no("empty_line_in_the_middle", HEADER + line("a") + "\n" + line("b"), "EFORMAT", nh + 2, "line")
    no("carriage_return_is_data", HEADER + line("a")[:-1] + "\r\n", "EFORMAT", nh + 1, "QUAL")
    ok("carriage_return_in_a_z_value", HEADER + line("a", aux=("co:Z:text",))[:-1] + "\r\n")
    # ---- field lengths around the 64-byte step
    ok("name_lengths", HEADER + "".join(line("n" * k, pos=k) for k in (1, 63, 64, 65, 254)))
    no("name_of_255", HEADER + line("ok") + line("n" * 255), "EFORMAT", nh + 2, "QNAME")
    seqs = ["*"] + [_bases(rng, k) for k in (1, 2, 63, 64, 65, 127, 128, 129)]
    seqs += ["acgtnACGTN", "=ACMGRSVTWYHKDBN" + "=acmgrsvtwyhkdbn", "AC.GT-ZU*x"]
    ok("seq_lengths_and_codes", HEADER + "".join(line("s%d" % k, pos=k + 1, seq=s) for k, s in enumerate(seqs)))
    ok("qual_missing_with_a_sequence", HEADER + line(seq=_bases(rng, 65), qual="*") + line(seq="A", qual="*"))
    no("qual_one_byte_short", HEADER + line(seq="ACGTA", qual="IIII"), "EFORMAT", nh + 1, "QUAL")
    no("qual_without_sequence", HEADER + line(seq="*", qual="II"), "EFORMAT", nh + 1, "QUAL")
    # ---- CIGAR
    ok("cigar_forms", HEADER + line("star", cigar="*") + "".join(line("op" + op, pos=k + 2, cigar="7" + op)
                                                                  for k, op in enumerate("MIDNSHP=X"))
       + line("mixed", cigar="3S10M2I4D1N5=1X6H2P9M") + line("longest", cigar="%dN" % (2 ** 28 - 1)))
    no("cigar_length_2_28", HEADER + line(cigar="%dN" % 2 ** 28), "EFORMAT", nh + 1, "CIGAR")
    no("cigar_length_0", HEADER + line(cigar="0M"), "EFORMAT", nh + 1, "CIGAR")
    no("cigar_without_length", HEADER + line(cigar="4MI"), "EFORMAT", nh + 1, "CIGAR")
    no("cigar_ends_in_digits", HEADER + line(cigar="4M3"), "EFORMAT", nh + 1, "CIGAR")
    no("cigar_unknown_op", HEADER + line(cigar="4Q"), "EFORMAT", nh + 1, "CIGAR")
    ok("cigar_65535_ops", HEADER + line(seq="*", cigar="1M2D" * 32767 + "3M"))
    no("cigar_65536_ops", HEADER + line(seq="*", cigar="1M2D" * 32768), "ERANGE", nh + 1, "CIGAR")
    # ---- aux
    ints = [-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1]
    ok("aux_integers", HEADER + line(aux=["i%x:i:%d" % (k, v) for k, v in enumerate(ints)]))
    no("aux_integer_2_32", HEADER + line(aux=["NM:i:%d" % 2 ** 32]), "EFORMAT", nh + 1, "aux")
    no("aux_integer_below_int32", HEADER + line(aux=["NM:i:%d" % (-2 ** 31 - 1)]), "EFORMAT", nh + 1, "aux")
    ok("aux_floats", HEADER + line(aux=["de:f:0.0123", "f1:f:1e-3", "f2:f:-2.5E+4", "f3:f:3", "f4:f:0", "f5:f:16777217"])
       + line("second", pos=5, aux=["dv:f:0.5"]))
    ok("aux_other_types", HEADER + line(aux=["tp:A:P", "ez:Z:", "cs:Z::10*ag:5 and : more", "hx:H:1AE301", "eh:H:"]))
    no("aux_type_b", HEADER + line(aux=["NM:i:1", "ba:B:c,1,2"]), "EFORMAT", nh + 1, "aux")
    no("aux_unknown_type", HEADER + line(aux=["xx:q:1"]), "EFORMAT", nh + 1, "aux")
    no("aux_too_short", HEADER + line(aux=["NM:i"]), "EFORMAT", nh + 1, "aux")
    no("aux_empty_after_trailing_tab", HEADER + line()[:-1] + "\t\n", "EFORMAT", nh + 1, "aux")
    ok("aux_40_fields", HEADER + line(aux=["%c%c:%s" % (97 + k // 26, 97 + k % 26, ("i:%d" % (k * 997), "Z:" + "v" * (k * 5),
                                                                                        "A:%c" % (65 + k % 26), "f:%d.5" % k)[k % 4])
                                           for k in range(40)]))
    no("ten_fields", HEADER + line("a") + "\t".join(line("b").split("\t")[:10]) + "\n", "EFORMAT", nh + 2, "line")
    no("flag_65536", HEADER + line(flag=65536), "EFORMAT", nh + 1, "FLAG")
    no("mapq_256", HEADER + line(mapq=256), "EFORMAT", nh + 1, "MAPQ")
    no("pos_signed", HEADER + line(pos="-1"), "EFORMAT", nh + 1, "POS")
    ok("tlen_ends", HEADER + line("lo", tlen=-2 ** 31) + line("hi", tlen=2 ** 31 - 1, pos=2 ** 31 - 1, rname="chr10"))
    no("tlen_2_31", HEADER + line(tlen=2 ** 31), "EFORMAT", nh + 1, "TLEN")
    # ---- names
    no("rname_unknown", HEADER + line("a") + line("b") + line("c", rname="chr11"), "EFORMAT", nh + 3, "RNAME", "'chr11'")
    no("rnext_unknown", HEADER + line("a", rnext="nope"), "EFORMAT", nh + 1, "RNEXT", "'nope'")
    ok("rnext_forms", HEADER + line("same", rnext="=", pnext=7) + line("none", pos=2) + line("named", pos=3, rnext="chr1b", pnext=1)
       + line("unmapped_mate_of", flag=4, rname="*", pos=0, rnext="=", pnext=0))
    ok("names_sharing_a_prefix", HEADER + line("p1", rname="chr10", pos=4) + line("p2", rname="chr1b", pos=3)
       + line("p3", rname="chr1", pos=2) + line("p4", rname="a" * 200, pos=1) + line("p5", rname="x|y:z"))
    many = ["ref_%d_%s" % (k, "x" * (k % 70)) for k in range(3000)]
    picks = rng.sample(range(3000), 300)
    ok("3000_references", "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, 1000 + k) for k, nm in enumerate(many))
       + "".join(line("m%d" % k, rname=many[k], pos=1 + k % 5, rnext=many[(k * 7) % 3000], pnext=3) for k in picks))
    no("duplicate_sn", "@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:5\n@SQ\tSN:a\tLN:6\n", "EFORMAT", 3, "@SQ")
    no("sq_without_ln", "@HD\tVN:1.6\n@SQ\tSN:a\n", "EFORMAT", 2, "@SQ")
    # ---- order
    ok("order_ties_strands_and_unmapped", HEADER + line("t1", pos=50) + line("rev", flag=16, pos=40) + line("fwd", pos=40)
       + line("t2", pos=50) + line("u1", flag=4, rname="*", pos=0) + line("pos0", pos=0) + line("placed", flag=4, rname="chr1", pos=45)
       + line("u2", flag=4, rname="*", pos=0) + line("t3", pos=50) + line("other", rname="chrM", pos=1) + line("u3", flag=4, rname="*", pos=0))
    for n in (1, 2, 255, 256, 257, 5000):
        ok("order_%d" % n, order_text(n, seed=n))
    return C
