"""Round 1 on a session opened from SAM text: region_split.filter_and_split_reads_by_region_cluster_from
and filter_split_and_extract_umis_from on Context.sam_open of shuffled SAM text, against the existing path-based
functions on the sorted BAM that tests/sam_ref.py makes of the same text -- the yardstick is the tested path, not the
code under test; and minimap2_align.minimap2_ont_align_session behind a stub `minimap2`."""
import collections
import json
import os
import random
import stat

import bam_ref
import numpy as np
import pytest
import sam_cases
import sam_ref
import split_extract_ref as ref
from test_bam_filter_cpu import report_of
from test_gpu_region_split import _mixed_records, _norm_log
from umiclust import _lib, minimap2_align
from umiclust import region_split as rs
from umiclust import vsearch_umi_cluster as _v

pytestmark = pytest.mark.gpu

EIO, EFORMAT, ESTATE = -5, -74, -77


def sam_text(refs, records, rng):
    """the record dicts of the region-split tests as SAM text, shuffled"""
    records = list(records)
    rng.shuffle(records)
    out = ["@HD\tVN:1.6\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in refs]
    for r in records:
        cigar = "".join("%d%s" % (ln, op) for op, ln in r["cigar"] if ln) or "*"  # (a length of 0 is no SAM)
        out.append(sam_cases.line(r["name"], r["flag"], refs[r["ref"]][0] if r["ref"] >= 0 else "*",
                                  r["pos"] + 1 if r["ref"] >= 0 else 0, cigar=cigar, seq=r["seq"] or "*", qual="*"))
    return "".join(out).encode()


def _read_dir(d):
    return {fn: open(os.path.join(d, fn), "rb").read() for fn in sorted(os.listdir(d))}


def both_ways(tmp_path, regions, clusters, records, seed, umi=None, **kw):
    """the session form on the text and the path form on the sorted BAM: (exception, returned names, files, logs) of
    each, which must be equal"""
    text = sam_text(regions, records, random.Random(seed))
    raw, _ = sam_ref.encode(text)
    got = []
    for tag in ("session", "path"):
        d = tmp_path / tag
        (d / "out").mkdir(parents=True), (d / "logs").mkdir()
        bam_ref.write_fasta(d / "ref.fa", regions)
        (d / "clusters.json").write_text(json.dumps(clusters))
        bam = str(d / "reads.bam")  # the session form only names its log after it
        args = (bam, str(d / "clusters.json"), str(d / "ref.fa"), str(d / "logs"), str(d / "out"))
        ret = err = None
        try:
            if tag == "path":
                bam_ref.write_bgzf(bam, raw, block=4096)
                ret = (rs.filter_split_and_extract_umis if umi else rs.filter_and_split_reads_by_region_cluster)(
                    *args, **kw, **(umi or {}))
            else:
                (d / "reads.sam").write_bytes(text)
                with _v.context().sam_open(d / "reads.sam") as src:
                    ret = (rs.filter_split_and_extract_umis_from if umi else
                           rs.filter_and_split_reads_by_region_cluster_from)(src, *args, **kw, **(umi or {}))
                assert not os.path.exists(bam)
        except (KeyError, _lib.UmiclustError) as e:
            err = (type(e).__name__, getattr(e, "code", None), str(e))
        got.append((err, sorted(os.path.basename(p) for p in ret) if ret is not None else None, _read_dir(d / "out"),
                    {fn: _norm_log(t.decode()) for fn, t in _read_dir(d / "logs").items()}))
    assert got[0] == got[1]
    return got[0]


KW = dict(minimal_region_overlap=0.9, max_softclip_5_end=120, max_softclip_3_end=100)
UMI = dict(adapter_length_5_end=40, adapter_length_3_end=36, max_pattern_dist=3)


def _planted(seed, n_mixed=400, n_planted=1200):
    rng = random.Random(seed)
    regions = [(f"TRBV{i}_{rng.randint(1, 9)}", rng.randint(30, 150)) for i in range(13)]
    clusters = {nm: i // 2 for i, (nm, _) in enumerate(regions[:12])}
    records = _mixed_records(rng, n_mixed, regions, 0.9, 220, never_passing={12})
    records += ref.planted_records(rng, n_planted, regions[:12], 40, 36, 3)
    return regions, clusters, records


def test_split_and_extract_from_the_session(tmp_path):
    """the record mix of test_gpu_split_extract's first test, shuffled SAM: the detected-UMI files, the log, the
    returned paths"""
    regions, clusters, records = _planted(11)
    err, ret, files, logs = both_ways(tmp_path, regions, clusters, records, 1, umi=UMI, **KW)
    # (the equality with the path-based call is the check; this only keeps it from comparing nothing with nothing)
    assert err is None and len(files) == 6 and ret and sum(t.count(b">") for t in files.values()) > 0
    assert list(logs) == ["reads_filter_and_split_reads_by_region_cluster.err"]


def test_split_from_the_session(tmp_path):
    """the record mix of test_gpu_region_split's first test: the region FASTA files, the log, the returned paths"""
    rng = random.Random(7)
    regions = [(f"TRBV{k}_{rng.randint(1, 9)}", rng.randint(30, 150)) for k in range(13)]
    clusters = {nm: k // 2 for k, (nm, _) in enumerate(regions[:12])}
    records = _mixed_records(rng, 3000, regions, 0.9, 35, never_passing={12})
    err, ret, files, logs = both_ways(tmp_path, regions, clusters, records, 2, minimal_region_overlap=0.9,
                                      max_softclip_5_end=20, max_softclip_3_end=15)
    assert err is None and len(files) == 6 and sum(t.count(b">") for t in files.values()) > 400
    assert sum(t.count(b"\nNone\n") for t in files.values()) > 2


@pytest.mark.parametrize("fused", [False, True])
def test_key_error_from_the_session(tmp_path, fused):
    """a passing record of a region without a cluster: the same KeyError with its name; the split has written the
    records before it, the fused call no file"""
    regions, clusters, records = _planted(8, 100, 300)
    records.append(dict(name="passes", flag=16, ref=12, pos=0, cigar=[("M", regions[12][1])], seq="A" * regions[12][1]))
    err, ret, files, logs = both_ways(tmp_path, regions, clusters, records, 3, umi=UMI if fused else None, **KW)
    assert err == ("KeyError", None, repr(regions[12][0])) and ret is None and logs == {}
    assert bool(files) == (not fused)


def test_white_space_refusal_from_the_session(tmp_path):
    regions, clusters = [("TRBV_e", 100)], {"TRBV_e": 0}
    records = [dict(name=nm, flag=0, ref=0, pos=0, cigar=[("M", 100)], seq="ACGTAC" + "CCCC" + "TTGGAA")
               for nm in ("fine", "two words")]
    umi = dict(adapter_length_5_end=12, adapter_length_3_end=12, max_pattern_dist=0, umi_fwd="ACGTAC", umi_rev="TTGGAA")
    err, ret, files, logs = both_ways(tmp_path, regions, clusters, records, 4, umi=umi, minimal_region_overlap=0.95)
    assert err[:2] == ("UmiclustError", EFORMAT) and "white space in the query name 'two words'" in err[2]
    assert files == {} and logs == {}


def _census_of(col):
    """the counters count_cs_tags builds, in plain Python over bam_ref.Columns, in the form report_of reads"""
    a, b, c = collections.Counter(), collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    for i, r in enumerate(col.records):
        if r.cls == 2 and col.cs[i] is not None:
            a[col.cs[i]] += 1
            b[col.cs[i]][col.ref_names[r.ref]] += 1
            c[col.cs[i]][(int(col.cols[i]) - int(col.nm[i])) / int(col.cols[i])] += 1
    return dict(cs_counter=list(a.items()), cs_region_counter=[list(b[k].items()) for k in a],
                cs_blast_id_counter=[list(c[k].items()) for k in a])


@pytest.mark.parametrize("params,with_bam", [(None, True), ("--cs=long", False)])
def test_minimap2_ont_align_session(tmp_path, monkeypatch, params, with_bam):
    """a stub `minimap2` first on PATH prints a prepared SAM: the argv it got is the reference's list, its stderr and
    the three cs-tag blocks are the log, the BAM is written only on request, and the session is open"""
    text = sam_cases.order_text(600, seed=31).encode()
    raw, roff = sam_ref.encode(text)
    (tmp_path / "prepared.sam").write_bytes(text)
    bindir, logs = tmp_path / "bin", tmp_path / "logs"
    bindir.mkdir(), logs.mkdir()
    stub = bindir / "minimap2"
    stub.write_text("#!/bin/sh\nprintf '%%s\\n' \"$@\" > %s; echo stub-stderr >&2; cat %s\n"
                    % (tmp_path / "argv.txt", tmp_path / "prepared.sam"))
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    bam = tmp_path / "lib1.bam" if with_bam else None
    src = minimap2_align.minimap2_ont_align_session("/data/lib1.fastq.gz", "/data/ref.fa", str(logs), 7,
                                                    minimap2_params=params, bam_file=bam)
    try:
        assert (tmp_path / "argv.txt").read_text().split("\n")[:-1] == [
            "-ax", "map-ont", "-k19", "-w 19", "-U50,500", "-g10k", "--end-bonus=10", "-t", "7", "--cap-kalloc", "500m",
            params or "--cs", "/data/ref.fa", "/data/lib1.fastq.gz"]
        col = bam_ref.Columns(raw)
        assert (logs / "lib1_minimap2.err").read_text() == "stub-stderr\n" + report_of(_census_of(col))
        assert os.listdir(logs) == ["lib1_minimap2.err"]
        assert src.n == len(roff) and np.array_equal(src.cs_group, col.cs_group)
        if with_bam:
            assert bam_ref.check_bgzf(bam) == raw
        else:
            assert sorted(os.listdir(tmp_path)) == ["argv.txt", "bin", "logs", "prepared.sam"]
    finally:
        src.close()


def test_session_errors(gpu_ctx, tmp_path):
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.sam_open(tmp_path / "missing.sam")
    assert e.value.code == EIO
    with _lib.Context(0) as fresh:  # no session has been opened on it
        out = tmp_path / "out"
        out.mkdir()
        for call in (lambda: fresh.region_split(None, ["a"], [10], [0], 0.95, 73, 68, str(out)),
                     lambda: fresh.region_split_extract(None, ["a"], [10], [0], 0.95, 73, 68, 73, 68, 3, "ACGT", "ACGT",
                                                        str(out))):
            with pytest.raises(_lib.UmiclustError) as e:
                call()
            assert e.value.code == ESTATE
        assert os.listdir(out) == []
