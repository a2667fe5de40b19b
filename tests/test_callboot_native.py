"""tests/native/callboot_check.cpp: the per-call bootstrap's lane functions (aardvark_amd/csrc/avk_callboot.inl) on arrays exactly as long as a launch makes them,
and the host routes' own code (aardvark_amd/csrc/avk_callboot_host.h: what avk_size_boot_tallies_host / avk_kind_boot_tallies_host run) on a tiny batch, built with -fsanitize=address,undefined and run as a program of its own, the way tests/test_boot_native.py runs boot_check.cpp (nothing is loaded into Python under
a sanitizer); and the rule's header compiled as plain C."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "plain.c"
    src.write_text('#include "%s"\nint main(void) { avk_size_spec s = {1, {5}}; return (avk_callboot_n_keys(AVK_CALLBOOT_SIZE, &s) == 2 && avk_callboot_n_keys(AVK_CALLBOOT_KIND, 0) == 9 &&\n'
                   '    AVK_CALLBOOT_AT(2, 7, 3, 9, 4, 5, 6) == ((((2 * 7 + 3) * 9 + 4) * 13 + 5) * 14 + 6) && avk_callboot_blocks_ok(17, 1000, 9) && !avk_callboot_blocks_ok(5, 4096, 16) &&\n'
                   '    !avk_callboot_blocks_ok(1, 4097, 1) && !avk_callboot_blocks_ok(1, 0, 9) && avk_boot_weight(1, 0, 100, 0) <= 12) ? 0 : 1; }\n'
                   % os.path.join(ROOT, "aardvark_amd", "csrc", "avk_callboot.h"))
    exe = str(tmp_path / "plain")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-x", "c", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-pedantic", "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "callboot_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "callboot_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "callboot_check: ok" in out.stdout
