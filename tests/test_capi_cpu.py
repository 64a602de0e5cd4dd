"""The C-ABI library: builds, loads, exports every symbol include/hutoken_amd.h declares,
and fails loudly (never computes) without a GPU.  No compute calls here."""
import os
import re

import pytest

import helpers as H
from hutoken_amd import _capi


def test_library_exports_every_declared_symbol():
    lib = _capi.load()
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(hutk_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations found"
    assert sorted(_capi.EXPORTS) == declared
    for name in declared:
        assert hasattr(lib, name), name


def test_header_cites_reference_interfaces():
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    for cite in ("src/lib.c:185-571", "src/lib.c:779-794", "src/lib.c:668-720", "include/hutoken/core.h:11"):
        assert cite in header


def test_no_gpu_means_loud_failure(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ents, sp = H.random_byte_vocab(1, n_merges=50)
    vp, spath = H.write_vocab(tmp_path, "v", ents, sp)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.Context(vp, spath, None, True)
    host = _capi.Context(vp, spath, None, True, device=-2)  # tables only
    import numpy as np
    with pytest.raises(RuntimeError, match="host-only"):
        host.encode_packed(np.frombuffer(b"abc", dtype=np.uint8), np.array([0, 3], dtype=np.int64))
    with pytest.raises(RuntimeError, match="host-only"):  # no device to add a second one to
        host.add_device(0)
    assert host.device_count == 0
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.Context(vp, spath, None, True, devices=[0, 1])


def test_debug_tile_kernel_follows_the_switches(tmp_path, monkeypatch):
    """hutk_debug_tile_kernel on host-only contexts (tables only, nothing is launched): which tile kernel a plain batch
    would be given, through the function the encode itself enqueues by.  Both switches are read on every call
    (HUTK_PTILES_MIN_TILES used to be read once per process); the default threshold is four tiles per workgroup of the
    persistent kernel's grid, which is at least 8 workgroups; the refusals are a vocabulary whose ids do not rise with the
    symbols (duplicate ids: rank_is_sym == 0) and character mode."""
    for k in ("HUTK_PTILES", "HUTK_PTILES_MIN_TILES", "HUTK_NO_SEAM"):
        monkeypatch.delenv(k, raising=False)
    tile = _capi.load().hutk_debug_tile_bytes()
    ents, sp = H.random_byte_vocab(1, n_merges=500)
    vp, spath = H.write_vocab(tmp_path, "t1", ents, sp)
    taken = _capi.Context(vp, spath, None, True, device=-2)
    ents, sp = H.random_byte_vocab(3, n_merges=500, dup_ids=True)
    vp, spath = H.write_vocab(tmp_path, "t3", ents, sp)
    refused = _capi.Context(vp, spath, None, True, device=-2)
    assert taken.table_stats()["rank_is_sym"] == 1 and refused.table_stats()["rank_is_sym"] == 0
    ents, sp = H.random_char_vocab(1, n_merges=300)
    vp, spath = H.write_vocab(tmp_path, "tc", ents, sp)
    chars = _capi.Context(vp, spath, "▁", False, device=-2)
    huge, small = 1 << 30, 31 * tile  # more tiles than 4 * any grid; fewer than 4 * 8
    assert taken.tile_kernel(huge) == 2 and taken.tile_kernel(small) == 0 and taken.tile_kernel(0) == 0
    monkeypatch.setenv("HUTK_PTILES", "1")
    assert taken.tile_kernel(huge) == 1 and taken.tile_kernel(small) == 0
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "1")  # (no new process, no new context)
    assert [taken.tile_kernel(n) for n in (0, 1, tile, tile + 1, small, huge)] == [0, 1, 1, 1, 1, 1]
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "3")
    assert [taken.tile_kernel(n) for n in (2 * tile, 2 * tile + 1)] == [0, 1]
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "1")
    monkeypatch.setenv("HUTK_PTILES", "0")
    assert taken.tile_kernel(1) == 0 and taken.tile_kernel(huge) == 0
    monkeypatch.delenv("HUTK_PTILES")
    assert taken.tile_kernel(1) == 2 and taken.tile_kernel(huge) == 2
    monkeypatch.setenv("HUTK_NO_SEAM", "1")  # without seams the device has nothing to choose by: k_tiles
    assert taken.tile_kernel(huge) == 0
    monkeypatch.setenv("HUTK_PTILES", "1")
    assert taken.tile_kernel(huge) == 1
    monkeypatch.delenv("HUTK_NO_SEAM")
    for ctx in (refused, chars):
        for mode in ("1", None):
            if mode is None:
                monkeypatch.delenv("HUTK_PTILES")
            assert ctx.tile_kernel(1) == 0 and ctx.tile_kernel(huge) == 0
        monkeypatch.setenv("HUTK_PTILES", "1")
    with pytest.raises(TypeError):
        taken.tile_kernel(-1)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(H.ROOT, "hutoken_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".c")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "hutk_oracle" not in src and "hto_" not in src, f
