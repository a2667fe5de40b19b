"""tests/native/unpack_calls_check.cpp: the per-call outputs by element (aardvark_amd/csrc/avk_devpack.inl: dp_unpack_calls) against the region-by-region dp_unpack
on arrays exactly as long as their contents, built with -fsanitize=address,undefined and run as a program of its own, the way tests/test_size_native.py runs
size_check.cpp (nothing is loaded into Python under a sanitizer).  The two functions are lane-local, so the program never starts a wave of tests/emu/wave_threads.h;
the compiler sees that and warns about the header's unused wave pointer, hence -Wno-nonnull."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "unpack_calls_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-strict-aliasing",
                           "-Wno-unused-parameter", "-Wno-nonnull", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "unpack_calls_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "unpack_calls_check: ok" in out.stdout
