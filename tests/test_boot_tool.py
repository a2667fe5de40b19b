"""aardvark_amd_compare --bootstrap: what the tool refuses, by name, before it reads a file or makes a context (no GPU needed).  The runs themselves are in
tests/test_gpu_boot.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSALS = [(["--bootstrap", "8", "--output-debug", "/nonexistent/dbg"], "--bootstrap cannot be combined with --output-debug"),
            (["--bootstrap", "8", "-s", "none.tsv", "--strat-lists", "host"], "cannot be combined with --strat-lists host"),
            (["--bootstrap", "4097"], "from 0 (off) to 4096"),
            (["--bootstrap", "x"], "invalid value for --bootstrap"),
            (["--bootstrap-seed", "3"], "need --bootstrap"),
            (["--bootstrap-level", "99"], "need --bootstrap"),
            (["--bootstrap", "8", "--bootstrap-level", "80"], "--bootstrap-level takes 90, 95 or 99"),
            (["--bootstrap", "8", "--bootstrap-seed", "1x"], "invalid value for --bootstrap-seed")]


def test_tool_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
    for extra, text in REFUSALS:
        r = subprocess.run([cli, "-r", "none.fa", "-t", "none.vcf", "-q", "none.vcf", "-o", str(tmp_path / "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 64 and text in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "out" / "summary_ci.tsv"))


def test_usage_names_the_options():
    cli = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_compare")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stderr for o in ("--bootstrap B", "--bootstrap-seed", "--bootstrap-level"))
