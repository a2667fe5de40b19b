"""The forms of an upload (csrc/avk_upload_forms.h) on the CPU: tests/native/upload_forms_check.cpp, a program of its own, built with the address and
undefined-behaviour sanitizers and run — hand-made batches in each of the five forms give the sizes, flags, argument checks (code and message), owned call
ranges, host-side allele offsets and slice picks that the upload's own expressions gave before the header, which the program keeps longhand as its reference."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_form_reads_as_the_upload_did(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/native/upload_forms_check.cpp")
    exe = str(tmp_path / "upload_forms_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "upload_forms_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "upload_forms_check: ok" in out.stdout
