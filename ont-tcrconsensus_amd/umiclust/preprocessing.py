"""Drop-in for the vsearch call of /root/reference/ont_tcr_consensus/preprocessing.py.

`vsearch_fastq_filtering` (:104-159) has the reference's name, signature, path rules and return value.  The
reference builds a `vsearch --fastq_filter` argv and runs it with `subprocess.run` (:129-148); here the *same argv*
is handed to the MI355X library through its C ABI (`umiclust_fastq_filter_argv`, include/umiclust.h), which parses it
with vsearch's option semantics (policies O7a-O7f) and writes the same filtered FASTQ and a log holding
vsearch's summary line.

Differences:
  * it does not run `seqkit`: the reference's two `seqkit stat -a` calls (:126-127, :156-157) write
    `<logs>/<name>_stats_before_vsearch_filtering.txt` and `..._after_...txt`; those files are not written here.
    A pipeline that reads them keeps the reference's function and replaces only its `subprocess.run([...vsearch...])`
    with `run_fastq_filter([...])`;
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


try:  # pragma: no cover - ray is not installed in this image
    import ray as _ray

    vsearch_fastq_filtering = _ray.remote(num_cpus=1)(_vsearch_fastq_filtering)
except ImportError:
    vsearch_fastq_filtering = _LocalRemote(_vsearch_fastq_filtering)
