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


_C_CLASSES = {"int": "int32", "int32_t": "int32", "uint32_t": "uint32", "int64_t": "int64", "uint64_t": "uint64",
              "size_t": "uint64", "float": "float", "void": "void"}


def _c_class(decl, is_return=False):
    """The class of one parameter (or return type) of a prototype: what a caller has to pass in that place."""
    decl = decl.strip()
    if "*" in decl or "[" in decl:
        base = decl.split("*")[0].replace("const", "").split()
        return "string" if base == ["char"] else "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words, "an empty declaration"
    if not is_return and len(words) > 1:
        words = words[:-1]  # (the parameter's name)
    assert len(words) == 1 and words[0] in _C_CLASSES, "a type this test does not know: %r" % decl
    return _C_CLASSES[words[0]]


def _ctypes_class(t):
    import ctypes as C
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "string"
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return "pointer"
    if t is C.c_float:
        return "float"
    assert issubclass(t, C._SimpleCData) and t._type_ in "iIlLqQ", "a ctypes type this test does not know: %r" % t
    return ("uint" if t._type_ in "ILQ" else "int") + str(8 * C.sizeof(t))


def header_prototypes():
    """name -> (class of the return type, [class of every parameter]) of every hutk_* prototype of the header"""
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t]*?[ \t*]+)\b(hutk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in protos, name
        ret = ret.replace("extern", "").strip()
        params = [p for p in (q.strip() for q in params.split(",")) if p]
        args = [] if params in ([], ["void"]) else [_c_class(p) for p in params]
        protos[name] = (_c_class(ret, is_return=True), args)
    return protos


def test_signatures_have_the_headers_types():
    """Every place of every ctypes signature is of the class the header declares: pointer, C string, 32-bit or 64-bit,
    signed or unsigned, float, void.  An int32 where the header says int64_t passes every small test and truncates
    a batch past 2^31; the test above compares names only."""
    import ctypes as C
    assert C.sizeof(C.c_int) == 4 and C.sizeof(C.c_size_t) == 8
    protos = header_prototypes()
    assert sorted(protos) == sorted(_capi.SIGNATURES), "the parser and the table do not list the same functions"
    wrong = []
    for name, (ret, args) in sorted(protos.items()):
        restype, argtypes = _capi.SIGNATURES[name]
        got = (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes])
        if got[0] != ret:
            wrong.append("%s returns %s, the table has %s" % (name, ret, got[0]))
        if len(got[1]) != len(args):
            wrong.append("%s takes %d arguments, the table has %d" % (name, len(args), len(got[1])))
            continue
        wrong += ["%s, argument %d: the header has %s, the table %s" % (name, i, a, g)
                  for i, (a, g) in enumerate(zip(args, got[1])) if a != g]
    assert not wrong, "\n".join(wrong)


def test_the_signature_parser_tells_the_classes_apart():
    """(the check of the check: a width, a sign or a count that differs is seen)"""
    import ctypes as C
    assert [_c_class(p) for p in ("const hutk_ctx* ctx", "const char* path", "int64_t n", "int flags", "uint32_t a3", "size_t n",
                                  "uint64_t seed", "float p", "const int64_t* d_offsets", "hutk_ctx** out", "double* out10")] \
        == ["pointer", "string", "int64", "int32", "uint32", "uint64", "uint64", "float", "pointer", "pointer", "pointer"]
    assert [_ctypes_class(t) for t in (C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.c_int32, C.c_uint32, C.c_size_t, C.c_uint64,
                                       C.c_float, C.POINTER(C.c_int64), None)] \
        == ["pointer", "string", "int64", "int32", "int32", "uint32", "uint64", "uint64", "float", "pointer", "void"]
    protos = header_prototypes()
    assert protos["hutk_ids_capacity"] == ("int64", ["pointer", "int64", "int64"])
    assert protos["hutk_host_alloc"] == ("pointer", ["uint64"]) and protos["hutk_last_error"] == ("string", [])
    assert protos["hutk_ctx_destroy"] == ("void", ["pointer"])


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
