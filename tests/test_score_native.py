"""tests/native/score_check.cpp: both score kernels' wave code (aardvark_amd/csrc/avk_score.inl) and the rule's header on arrays exactly as long as a launch makes
them, against a restatement of the rule, built with -fsanitize=address,undefined and run as a program of its own, the way tests/test_size_native.py runs
size_check.cpp (nothing is loaded into Python under a sanitizer)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "score_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", "score_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "score_check: ok" in out.stdout
