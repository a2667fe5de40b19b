"""aardvark_amd_compare --roc QUAL|GQ [--roc-thresholds a,b,..]: what the tool refuses, by name and with exit code 64, before it reads a file or makes a context,
and what --help says.  No GPU needed; the runs are in tests/test_gpu_score.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
LIST_TEXT = "--roc-thresholds takes 1 to 31 finite, strictly ascending numbers"
REFUSALS = [(["--roc", "QUAL", "--roc-thresholds", "5,5"], LIST_TEXT),
            (["--roc", "QUAL", "--roc-thresholds", "10,5"], LIST_TEXT),
            (["--roc", "QUAL", "--roc-thresholds", "1,x"], LIST_TEXT),
            (["--roc", "QUAL", "--roc-thresholds", "1,,2"], LIST_TEXT),
            (["--roc", "QUAL", "--roc-thresholds", ""], LIST_TEXT),
            (["--roc", "GQ", "--roc-thresholds", "1,nan"], LIST_TEXT),
            (["--roc", "GQ", "--roc-thresholds", "1,inf"], LIST_TEXT),
            (["--roc", "GQ", "--roc-thresholds", ",".join(str(k) for k in range(32))], LIST_TEXT),
            (["--roc-thresholds", "1,6"], "--roc-thresholds needs --roc"),
            (["--roc", "DP"], "unknown field: DP"),
            (["--roc", "qual"], "unknown field: qual"),
            (["--roc", "QUAL", "--output-debug", "/nonexistent/dbg"], "--roc cannot be combined with --output-debug"),
            (["--roc", "GQ", "-s", "none.tsv", "--strat-lists", "host"], "--roc on the packed feed reads the labels from the sets on the GPU: it cannot be combined with --strat-lists host")]


def test_tool_refusals_need_no_device(tmp_path):
    for extra, text in REFUSALS:
        r = subprocess.run([CLI, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))  # (refused before anything is made, the output folder included)


def test_a_valid_list_passes_the_option_checks(tmp_path):
    """31 thresholds, negative and fractional ones: the refusal that follows is about the input files, not the options"""
    r = subprocess.run([CLI, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out"), "--roc", "GQ", "--roc-thresholds",
                        ",".join("%g" % (k - 2.5) for k in range(31))], capture_output=True, text=True)
    assert r.returncode not in (0, 64) and "--roc" not in r.stderr


def test_usage_names_the_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stderr for o in ("--roc QUAL|GQ", "--roc-thresholds", "summary_roc.tsv", "5,10,15,20,25,30,35,40,50,60"))
    assert "approximation of a filtered re-run" in r.stderr
