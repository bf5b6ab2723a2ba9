"""The host arithmetic of the frame check (comms_rs_amd/csrc/crc_tables.hpp: x^n mod P, the word remainder, the multiply mod P
and the word-parallel combination the kernels of crc.hip form) against the bit-serial register, on the CPU:
tests/crc_tables_test.cpp includes only that header, is built with AddressSanitizer and UBSan and run as a program of its
own.  Widths 1, 5, 8, 16, 24, 32; lengths 1 ... 200, 2047, 2048, 2049, 65504, 65535 and 2^16 - W; zero and non-zero init."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crc_tables_under_sanitizers(tmp_path):
    exe = str(tmp_path / "crc_tables_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "comms_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "crc_tables_test.cpp"), "-o", exe], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
