"""Drop-ins for ont_tcr_consensus/count.py: count_sequences_in_fasta (:9-20), umi_counter
(:23-36) and write_region_umi_counts_to_csv (:39-51), the last call of the per-library loop (tcr_consensus.py:453-458).

Same signatures, the same umi_consensus_counts.csv and the same RuntimeError texts, without `grep` and without pandas:
the `>` lines are counted in-process and the CSV is written as DataFrame.to_csv(index=False) writes it.  Host-only
file work; nothing here touches the device.  When `ray` is importable count_sequences_in_fasta is a `ray.remote` task
like the reference's; without ray `.remote(...)` runs in-process.  Pinned by tests/golden/count, which the
reference's own functions produced.
"""
from __future__ import annotations

import csv
import os
from typing import Union

from .vsearch_umi_cluster import _LocalRemote


def _count_sequences_in_fasta(smolecule_fa):
    """:9-20 -- the number of lines that start with `>`, as `grep -c "^>"` prints it.  grep exits 1 when it counts
    none and 2 when it cannot read the file; the reference turns either into a RuntimeError, wrapped once more by
    its own `except Exception`."""
    try:
        try:
            with open(smolecule_fa, "rb") as fh:
                data = fh.read()
        except OSError as e:
            raise RuntimeError(f"Error processing {smolecule_fa}: grep: {smolecule_fa}: {e.strerror}")
        count = int(data.startswith(b">")) + data.count(b"\n>")
        if count:
            return count
        raise RuntimeError(f"Error processing {smolecule_fa}: ")  # grep's exit status 1, nothing on stderr
    except Exception as e:
        raise RuntimeError(f"Exception occurred while processing {smolecule_fa}: {e}")


try:  # pragma: no cover - ray is not installed in this image
    import ray as _ray

    count_sequences_in_fasta = _ray.remote(num_cpus=1)(_count_sequences_in_fasta)
    _get = _ray.get
except ImportError:
    count_sequences_in_fasta = _LocalRemote(_count_sequences_in_fasta)

    def _get(values):
        return values


def umi_counter(smolecule_filtered_fa_list: list):
    """:23-36 -- {region: count}, the region being what follows `region_` in the file's directory"""
    region_umi_counter = {}
    futures = [count_sequences_in_fasta.remote(smolecule_fa) for smolecule_fa in smolecule_filtered_fa_list]
    for smolecule_fa, count in zip(smolecule_filtered_fa_list, _get(futures)):
        region_umi_counter[os.path.dirname(smolecule_fa).split("region_")[1]] = count
    return region_umi_counter


def write_region_umi_counts_to_csv(smolecule_filtered_fa_list: list,
                                   library_umi_counts_dir: Union[str, os.PathLike[str]], region_name: str = "TCR"):
    """:39-51 -- <library_umi_counts_dir>/umi_consensus_counts.csv with the columns region_name and Count"""
    umi_counts_csv = os.path.join(library_umi_counts_dir, "umi_consensus_counts.csv")
    region_umi_counter = umi_counter(smolecule_filtered_fa_list=smolecule_filtered_fa_list)
    with open(umi_counts_csv, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")  # DataFrame.to_csv(index=False): minimal quoting
        w.writerow([region_name, "Count"])
        w.writerows(region_umi_counter.items())
