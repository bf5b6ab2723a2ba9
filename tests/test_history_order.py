"""The layout conversion of the nodes' sample history (comms_rs_amd/csrc/history_order.hpp: reference state, newest
first <-> device ring, time order), on the CPU: tests/history_order_test.cpp includes only that header, is built with
AddressSanitizer and UBSan and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_history_order_under_sanitizers(tmp_path):
    exe = str(tmp_path / "history_order_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "comms_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "history_order_test.cpp"), "-o", exe], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
