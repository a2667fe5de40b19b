"""aardvark_amd_merge --sweep: one solve, the outputs of several strategies.  Every strategy's files are compared with a separate run of the tool as it is without the
option (--merge-strategy <name>), on the small job the other tool tests write (tests/test_merge_outputs.py: write_case)."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "aardvark_amd", "bin", "aardvark_amd_merge")


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True)


@pytest.mark.gpu
def test_a_sweep_writes_what_three_separate_runs_write(tmp_path):
    from test_merge_outputs import write_case
    p, _ = write_case(tmp_path, 1500, 600_000)
    base = ["-r", p["fa"]] + [x for v in p["vcfs"] for x in ("-i", v)] + ["-b", p["bed"], "--conflict-select", "1"]
    names = ["exact", "majority", "all"]
    strip = lambda x: b"\n".join(l for l in x.split(b"\n") if not l.startswith(b"##aardvark_command"))
    body = lambda x: [l for l in x.split(b"\n") if not l.startswith(b"#")]
    single = {}
    for name in names:  # the command line as it is without the option
        out, summary = str(tmp_path / ("one_" + name)), str(tmp_path / ("one_%s.tsv" % name))
        r = run(base + ["-o", out, "--output-summary", summary, "--merge-strategy", name])
        assert r.returncode == 0, r.stderr
        single[name] = (out, summary, [l for l in r.stderr.splitlines() if l.startswith("Solved:error")])
    # (--batch-regions 400: several calls of the sweep; --summary-counts device: the counters of every strategy come back with them, host: the per-region writer)
    for tag, extra in (("a", []), ("b", ["--batch-regions", "400", "--summary-counts", "device", "--contexts", "1"])):
        swept = str(tmp_path / ("swept_" + tag))
        r = run(base + ["-o", swept, "--output-summary", str(tmp_path / ("swept_%s.tsv" % tag)), "--sweep", ",".join(names), "-v"] + extra)
        assert r.returncode == 0, r.stderr
        assert "one solve served 3 strategies" in r.stderr and ("by kernel with the call" in r.stderr) == (tag == "b")
        assert sorted(os.listdir(swept)) == sorted(names)
        solved = [l for l in r.stderr.splitlines() if l.startswith("Solved:error")]
        for name in names:
            out, summary, single_solved = single[name]
            assert solved and solved == single_solved
            for f in ("regions.bed.gz", "failed_regions.bed.gz"):
                assert open(os.path.join(swept, name, f), "rb").read() == open(os.path.join(out, f), "rb").read(), (name, f)
            x, y = (gzip.open(os.path.join(d, "passing.vcf.gz"), "rb").read() for d in (os.path.join(swept, name), out))
            assert body(x) == body(y) and strip(x) == strip(y) and len(x) > 100, name  # (the header carries the command line: compared without that line)
            got = open(str(tmp_path / ("swept_%s.%s.tsv" % (tag, name))), "rb").read()
            assert got == open(summary, "rb").read() != b"", name
        # the strategies are not one and the same on this job
        assert len({open(os.path.join(swept, name, "regions.bed.gz"), "rb").read() for name in names}) == 3


def test_what_a_sweep_does_not_go_with(tmp_path):
    """refused from the command line, before any file is read and before the GPU is looked for (so this one needs none)"""
    base = ["-r", "none.fa", "-i", "a.vcf.gz", "-i", "b.vcf.gz", "-o", str(tmp_path / "x")]
    for extra in (["--sweep", "exact,all", "--merge-strategy", "all"], ["--merge-strategy", "exact", "--sweep", "exact"], ["--sweep", "exact,all", "--enable-voting"],
                  ["--sweep", "exact,all", "--enable-no-conflict"], ["--sweep", "exact,all", "--devices", "0,0"], ["--sweep", "exact,all", "--contexts", "2"],
                  ["--sweep", ""], ["--sweep", "exact,,all"], ["--sweep", "exact,best"], ["--sweep", "all,all"], ["--sweep", "exact", "--batch-form", "wide"]):
        r = run(base + extra)
        assert r.returncode == 64 and "error:" in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "x"))
