"""Host check of the start-bit arithmetic of k_tiles' word rounds (hutoken_amd/csrc/hutk_wordbits.h: "followed directly by
a start" and "next start within the table key") against a per-position loop -- tests/cpu/wordbits_check.cpp, built with
the address and undefined-behaviour sanitizers and run as a program of its own."""
import os
import subprocess

import helpers as H


def test_start_bit_arithmetic_matches_a_per_position_loop(tmp_path):
    exe = os.path.join(str(tmp_path), "wordbits_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cpu", "wordbits_check.cpp")])
    for n, seed in ((200000, 1), (200000, 2)):
        out = subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "mismatches 0" in out.stdout, out.stdout
