"""Drop-in for the vsearch call of /root/reference/ont_tcr_consensus/preprocessing.py.

`vsearch_fastq_filtering` (:104-159) has the reference's name, signature, path rules and return value.  The
reference builds a `vsearch --fastq_filter` argv and runs it with `subprocess.run` (:129-148); here the *same argv*
is handed to the MI355X library through its C ABI (`umiclust_fastq_filter_argv`, include/umiclust.h), which parses it
with vsearch's option semantics (policies O7a-O7f) and writes the same filtered FASTQ and a log holding
vsearch's summary line.

The reference's function also runs `seqkit stat -a` on the raw FASTQ before the filter (:126-127) and on the filtered
FASTQ after it (:156-157), into `<logs>/<name>_stats_before_vsearch_filtering.txt` and `..._after_...txt`;
`analysis.py:76-81` reads their AvgQual column.  `vsearch_fastq_filtering_with_stats` writes both tables from the
filter's own pass over the reads (`umiclust_fastq_filter_stats_argv`, row f5b, policy O8 of DESIGN.md §9a), so
preprocessing needs neither vsearch nor seqkit and reads the raw FASTQ once.  `vsearch_fastq_filtering` is the filter
alone and writes no tables.

Differences:
  * the tables restate seqkit >= 2.8.2's `stat -a` text (policy O8); the "before" table describes exactly the records
    the filter read and the "after" table exactly the records it wrote;
  * failures raise `UmiclustError` (the reference returns the output path even when vsearch fails, since
    `subprocess.run` has no `check=`).

When `ray` is importable the function is a `ray.remote` task like the reference's; without ray the same call syntax
(`f.remote(...)`, `f.options(...).remote(...)`, `f(...)`) runs synchronously in-process.
"""
from __future__ import annotations

import os
from typing import Union

from .vsearch_umi_cluster import _LocalRemote, context


def fastq_filter_argv(fastq, filtered_fastq, log_file, max_ee_rate_base, minimal_length) -> list[str]:
    """The argv of preprocessing.py:129-148, element for element."""
    return ["vsearch", "--fastq_filter", fastq, "--fastq_ascii", "33", "--fastq_qmax", "93", "--fastq_maxee_rate",
            str(max_ee_rate_base), "--fastq_minlen", str(minimal_length), "--quiet", "--log", log_file, "-fastqout",
            filtered_fastq]


def run_fastq_filter(argv: list[str]) -> dict:
    """Runs a `vsearch --fastq_filter` argv through the library; returns the result counters and phase times."""
    return context().fastq_filter_argv([os.fspath(a) for a in argv])


def run_fastq_filter_stats(argv: list[str], stats_before_txt, stats_after_txt) -> dict:
    """Runs a `vsearch --fastq_filter` argv through the library and writes the two `seqkit stat -a` tables
    (preprocessing.py:126-127, :156-157) from the same pass; returns the result counters, the phase times and
    "before" / "after", the tables' numbers."""
    return context().fastq_filter_stats_argv([os.fspath(a) for a in argv], os.fspath(stats_before_txt),
                                             os.fspath(stats_after_txt))


def _vsearch_fastq_filtering(
    fastq: Union[str, os.PathLike[str]],
    library_fastq_out_dir_dict: dict,
    library_logs_dir_dict: dict,
    max_ee_rate_base: float,
    minimal_length: int,
):
    """preprocessing.py:104-159 without its seqkit calls: filters `fastq` into
    `<fastq_out_dir>/<name>_filtered.fastq`, logs to `<logs_dir>/<name>_vsearch_fastq_filtering.log` and returns the
    filtered FASTQ's path.  The seqkit statistics files of the reference are not written."""
    fastq = os.fspath(fastq)
    lib_name = os.path.basename(os.path.dirname(fastq))  # the library is the FASTQ's directory name (:112)
    stem = os.path.basename(fastq).split(".")[0]
    filtered_fastq = os.path.join(library_fastq_out_dir_dict[lib_name], stem + "_filtered.fastq")
    log_file = os.path.join(library_logs_dir_dict[lib_name], stem + "_vsearch_fastq_filtering.log")
    run_fastq_filter(fastq_filter_argv(fastq, filtered_fastq, log_file, max_ee_rate_base, minimal_length))
    return filtered_fastq


def _vsearch_fastq_filtering_with_stats(
    fastq: Union[str, os.PathLike[str]],
    library_fastq_out_dir_dict: dict,
    library_logs_dir_dict: dict,
    max_ee_rate_base: float,
    minimal_length: int,
):
    """preprocessing.py:104-159 whole: the filter as above and the reference's two statistics files,
    `<logs_dir>/<name>_stats_before_vsearch_filtering.txt` (:118, :126-127) and
    `<logs_dir>/<name>_stats_after_vsearch_filtering.txt` (:156-157), written from the filter's pass."""
    fastq = os.fspath(fastq)
    lib_name = os.path.basename(os.path.dirname(fastq))
    stem = os.path.basename(fastq).split(".")[0]
    logs = library_logs_dir_dict[lib_name]
    filtered_fastq = os.path.join(library_fastq_out_dir_dict[lib_name], stem + "_filtered.fastq")
    log_file = os.path.join(logs, stem + "_vsearch_fastq_filtering.log")
    run_fastq_filter_stats(fastq_filter_argv(fastq, filtered_fastq, log_file, max_ee_rate_base, minimal_length),
                           os.path.join(logs, stem + "_stats_before_vsearch_filtering.txt"),
                           os.path.join(logs, stem + "_stats_after_vsearch_filtering.txt"))
    return filtered_fastq


try:  # pragma: no cover - ray is not installed in this image
    import ray as _ray

    vsearch_fastq_filtering = _ray.remote(num_cpus=1)(_vsearch_fastq_filtering)
    vsearch_fastq_filtering_with_stats = _ray.remote(num_cpus=1)(_vsearch_fastq_filtering_with_stats)
except ImportError:
    vsearch_fastq_filtering = _LocalRemote(_vsearch_fastq_filtering)
    vsearch_fastq_filtering_with_stats = _LocalRemote(_vsearch_fastq_filtering_with_stats)
