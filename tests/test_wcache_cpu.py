"""Host fuzz of the word cache's shared header (hutoken_amd/csrc/hutk_wcache.h: slot layout, key packing, hash) with a
host model of the kernels' insert and lookup -- tests/cpu/wcache_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program of its own."""
import os
import subprocess

import helpers as H


def test_word_cache_layout_and_host_model(tmp_path):
    exe = os.path.join(str(tmp_path), "wcache_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cpu", "wcache_check.cpp")])
    # (keys, seed, log2 of the buckets): a roomy table, a crowded one, one that overflows
    for n_keys, seed, log2 in ((20000, 1, 16), (20000, 2, 13), (5000, 3, 4)):
        out = subprocess.run([exe, str(n_keys), str(seed), str(log2)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "mismatches 0" in out.stdout, out.stdout
