"""ctypes binding of include/hutoken_amd.h (the C-ABI shared library).

The library is built in-tree (hutoken_amd/lib/libhutoken_amd.so).  Nothing here
computes token ids: if the library or a GPU is missing the calls raise.
"""
import ctypes as C
import importlib.util
import os
import sys

from . import build as _build

OK = 0
E_FILE_NOT_FOUND, E_VALUE, E_MEMORY, E_ARG, E_DEVICE, E_UNSUPPORTED = 1, 2, 3, 4, 5, 6
E_CAPACITY, E_NUL_BYTE, E_WORD_TOO_LARGE, E_INVALID_UTF8 = 7, 8, 9, 10
DOC_OK, DOC_WORD_TOO_LARGE, DOC_INVALID_UTF8 = 0, 1, 2
DOC_ID_OUT_OF_RANGE, DOC_ID_UNDECODABLE, DOC_SPAN_MISMATCH = 3, 4, 5

_vp, _i64, _i32, _s32, _u32, _str = C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_uint32, C.c_char_p
_pvp, _pi64, _ps32, _pf = C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_s32), C.POINTER(C.c_float)
_DEV = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp]  # the *_batch_device forms of both directions; with flags below
_DEV_F = [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _vp]
_HOST = [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]  # the host-buffer forms of both directions; with flags below
_HOST_F = [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp]
# every symbol include/hutoken_amd.h declares: name -> (restype, argtypes).  load() applies it, so a declared symbol
# cannot go without a signature (without argtypes ctypes truncates 64-bit arguments silently).
SIGNATURES = {
    "hutk_ctx_create": (_i32, [_pvp, _str, _str, _str, _i32, _i32]),
    "hutk_ctx_create_merges": (_i32, [_pvp, _str, _str, _str, _i32, _str, _i32]),
    "hutk_ctx_set_pattern": (_i32, [_vp, _str]),
    "hutk_ctx_set_pretokenizer": (_i32, [_vp, _i32, _vp, _i64]),
    "hutk_ctx_pretokenizer": (_i32, [_vp]),
    "hutk_ctx_add_device": (_i32, [_vp, _i32]),
    "hutk_ctx_device_count": (_i32, [_vp]),
    "hutk_uses_merges": (_i32, [_vp]),
    "hutk_ctx_destroy": (None, [_vp]),
    "hutk_last_error": (_str, []),
    "hutk_ids_capacity": (_i64, [_vp, _i64, _i64]),
    "hutk_encode_batch": (_i32, _HOST),
    "hutk_encode_batch_device": (_i32, _DEV),
    "hutk_encode": (_i32, [_vp, _vp, _i64, _vp, _i64, _pi64, _ps32]),
    "hutk_vocab_size": (_i64, [_vp]),
    "hutk_host_alloc": (_vp, [C.c_size_t]),
    "hutk_host_free": (None, [_vp]),
    "hutk_decode_batch": (_i32, _HOST),
    "hutk_decode_batch_device": (_i32, _DEV),
    "hutk_pair_table_entries": (_i64, [_vp]),
    "hutk_device_ordinal": (_i32, [_vp]),
    "hutk_table_stats": (_i32, [_vp, _vp]),
    "hutk_last_timing": (_i32, [_vp, _pf, _pf]),
    "hutk_set_timing": (None, [_vp, _i32]),
    "hutk_debug_pairs_second": (_i64, [_vp]),
    "hutk_debug_long_words": (_i64, [_vp]),
    "hutk_debug_profile": (_i32, [_vp, _i32]),
    "hutk_debug_profile_read": (_i32, [_vp, _i64, _vp]),
    "hutk_debug_profile_raw": (_i32, [_vp, _i64, _vp]),
    "hutk_debug_tile_bytes": (_i32, []),
    "hutk_debug_seam": (_i32, [_vp, _vp]),
    "hutk_debug_seam2_cut": (_i32, [_vp, _u32, _u32]),
    "hutk_debug_tile_kernel": (_i32, [_vp, _i64]),
    "hutk_debug_exc_counts": (_i32, [_vp, _vp]),
    "hutk_ctx_word_cache_stats": (_i32, [_vp, _vp]),
    "hutk_ctx_word_cache_clear": (_i32, [_vp]),
    "hutk_trainer_create": (_i32, [_pvp, _i32]),
    "hutk_trainer_add": (_i32, [_vp, _vp, _vp, _i64]),
    "hutk_trainer_run": (_i32, [_vp, _s32, _vp, _vp, _ps32]),
    "hutk_trainer_stats": (_i32, [_vp, _vp]),
    "hutk_trainer_destroy": (None, [_vp]),
    "hutk_trainer_debug_counters": (_i32, [_vp, _vp, _i32]),
    "hutk_trainer_create_mode": (_i32, [_pvp, _i32, _i32]),
    "hutk_trainer_alphabet": (_i32, [_vp, _vp, _i64, _vp, _i64, _pi64, _pi64]),
    "hutk_collate_padded_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _s32, _s32, _s32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hutk_packer_create": (_i32, [_pvp, _i64, _s32, _s32, _s32, _i32, _i32]),
    "hutk_packer_rows": (_i64, [_vp, _i64, _i64]),
    "hutk_packer_add_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _pi64, _vp, _vp]),
    "hutk_packer_flush_device": (_i32, [_vp, _vp, _vp, _vp, _pi64, _vp]),
    "hutk_packer_pending": (_i64, [_vp]),
    "hutk_packer_destroy": (None, [_vp]),
    "hutk_packer_create_channels": (_i32, [_pvp, _i64, _s32, _s32, _s32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "hutk_packer_channel_count": (_i32, [_vp]),
    "hutk_packer_add_channels_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _pi64, _vp, _vp]),
    "hutk_packer_flush_channels_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _pi64, _vp]),
    "hutk_packed_cu_seqlens_device": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hutk_packed_labels_device": (_i32, [_vp, _i32, _vp, _i64, _i64, _i32, _i64, _vp, _vp]),
    "hutk_debug_cu_tile": (_i32, []),
    "hutk_bestfit_rows_bound": (_i64, [_i64, _i64, _i64, _i32]),
    "hutk_bestfit_plan_device": (_i32, [_vp, _i64, _i64, _i64, _s32, _s32, _i64, _vp, _vp, _vp, _vp]),
    "hutk_bestfit_rows_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _s32, _s32, _s32, _i32, _i64, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp]),
    "hutk_rows_gather_source_device": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i64, _vp, _vp, _vp]),
    "hutk_debug_bestfit_tile": (_i32, []),
    "hutk_token_spans_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "hutk_token_spans": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "hutk_debug_span_tile_ids": (_i32, []),
    "hutk_debug_span_chunk_bytes": (_i32, []),
    "hutk_ctx_set_special_tokens": (_i32, [_vp, _vp, _vp, _vp, _i64]),
    "hutk_ctx_special_token_count": (_i64, [_vp]),
    "hutk_special_ids_capacity": (_i64, [_vp, _i64, _i64]),
    "hutk_encode_special_batch_device": (_i32, _DEV),
    "hutk_encode_special_batch": (_i32, _HOST),
    "hutk_special_last_matches": (_i64, [_vp]),
    "hutk_debug_special_tile_bytes": (_i32, []),
    "hutk_decode_special_batch_device": (_i32, _DEV_F),
    "hutk_decode_special_batch": (_i32, _HOST_F),
    "hutk_ctx_find_byte_tokens": (_i32, [_vp, _vp]),
    "hutk_ctx_set_byte_fallback": (_i32, [_vp, _vp]),
    "hutk_ctx_byte_fallback": (_i32, [_vp, _vp]),
    "hutk_encode_fallback_batch_device": (_i32, _DEV_F),
    "hutk_encode_fallback_batch": (_i32, _HOST_F),
    "hutk_decode_fallback_batch_device": (_i32, _DEV_F),
    "hutk_decode_fallback_batch": (_i32, _HOST_F),
    "hutk_windows_rows_bound": (_i64, [_i64, _i64, _i64, _i64, _i32]),
    "hutk_windows_rows_device": (_i32, [_vp, _i64, _i64, _i64, _i64, _s32, _s32, _vp, _vp, _vp]),
    "hutk_collate_windows_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _s32, _s32, _s32, _i32, _i32,
                                           _vp, _vp, _vp, _vp, _vp, _vp]),
    "hutk_pair_rows_bound": (_i64, [_i64, _i64, _i64, _i64, _i32]),
    "hutk_pair_rows_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _s32, _vp, _i32, _s32, _vp, _vp, _vp]),
    "hutk_collate_pairs_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _s32, _vp,
                                         _i32, _s32, _s32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hutk_normalizer_create": (_i32, [_pvp, _i32, _vp, _i64]),
    "hutk_normalizer_destroy": (None, [_vp]),
    "hutk_normalizer_info": (_i32, [_vp, _vp]),
    "hutk_normalize_batch_device": (_i32, [_vp, _i32, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hutk_normalize_batch": (_i32, [_vp, _i32, _vp, _vp, _i64, _pvp, _pvp]),
    "hutk_pretokenizer_create": (_i32, [_pvp, _i32, _vp, _i64]),
    "hutk_pretokenizer_destroy": (None, [_vp]),
    "hutk_pretokenize_batch_device": (_i32, [_vp, _i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "hutk_pretokenize_starts_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hutk_debug_norm_chunk_bytes": (_i32, []),
    "hutk_debug_presplit_chunk_bytes": (_i32, []),
    "hutk_padded_plan_device": (_i32, [_vp, _i64, _i64, _i64, _s32, _s32, _i32, _vp, _vp, _vp]),
    "hutk_windows_plan_device": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _s32, _s32, _i32, _vp, _vp, _vp]),
    "hutk_pair_plan_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _s32, _vp, _i32, _s32, _i32,
                                     _vp, _vp, _vp]),
    "hutk_rows_gather_device": (_i32, [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hutk_token_word_ids_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hutk_debug_word_ids_tile": (_i32, []),
    "hutk_rows_answers_device": (_i32, [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp]),
    "hutk_rows_mlm_device": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _i64, C.c_uint64, _i64, _i64, _i64, _s32, _i64,
                                    _i64, _i32, _vp, _vp, _vp, _vp]),
    "hutk_rows_labels_device": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp]),
    "hutk_rows_span_corrupt_device": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, C.c_uint64, _i64, _vp, _i32, _i64, _i32, _i64,
                                             _s32, _s32, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hutk_chat_template_create": (_i32, [_pvp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _s32, _s32]),
    "hutk_chat_template_destroy": (None, [_vp]),
    "hutk_chat_ids_bound": (_i64, [_vp, _i64, _i64, _i64, _i32]),
    "hutk_chat_offsets_device": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hutk_chat_render_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _u32, _s32, _i64,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "hutk_debug_chat_span": (_i32, []),
    "hutk_fim_ids_bound": (_i64, [_i64, _i64, _i32]),
    "hutk_fim_cut_text_device": (_i32, [_vp, _vp, _i64, _i64, C.c_uint64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hutk_fim_plan_tokens_device": (_i32, [_vp, _i64, _i64, C.c_uint64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hutk_fim_plan_pieces_device": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hutk_fim_render_device": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _s32, _s32, _s32, _s32, _u32, _s32, _i64, _vp, _vp, _vp,
                                      _vp, _vp, _vp]),
    "hutk_debug_fim_span": (_i32, []),
    "hutk_debug_fim_decide": (_i32, [C.c_uint64, _i64, _i64, _i64, _i64, _pi64]),
    "hutk_debug_fim_locate": (_i32, [_i64, _i64, _i64, _i32, _i32, _i64, _pi64]),
    "hutk_wordpiece_create": (_i32, [_pvp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _str, _str, _s32, _u32]),
    "hutk_wordpiece_destroy": (None, [_vp]),
    "hutk_wordpiece_info": (_i32, [_vp, _vp]),
    "hutk_wordpiece_ids_capacity": (_i64, [_vp, _i64, _i64]),
    "hutk_wordpiece_encode_batch_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hutk_wordpiece_encode_batch": (_i32, [_vp, _vp, _vp, _i64, _pvp, _pvp, _pvp]),
    "hutk_debug_wordpiece_chunk_bytes": (_i32, []),
    "hutk_debug_wordpiece_bucket": (_i64, [_vp, _vp, _i64, _i32]),
    "hutk_unigram_create": (_i32, [_pvp, _i32, _vp, _vp, _vp, _i64, _i64, _u32]),
    "hutk_unigram_destroy": (None, [_vp]),
    "hutk_unigram_info": (_i32, [_vp, _vp]),
    "hutk_unigram_ids_capacity": (_i64, [_vp, _i64, _i64]),
    "hutk_unigram_encode_batch_device": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hutk_unigram_encode_batch": (_i32, [_vp, _vp, _vp, _i64, _pvp, _pvp, _pvp]),
    "hutk_debug_unigram_chunk_bytes": (_i32, []),
    "hutk_debug_unigram_bucket": (_i64, [_vp, _vp, _i64]),
}
EXPORTS = list(SIGNATURES)
TRAIN_BYTES, TRAIN_CHARS = 0, 1
COLLATE_TRUNC_LEFT, COLLATE_PAD_LEFT = 1, 2
NO_TOKEN = -2**31  # HUTK_NO_TOKEN: "no bos / no eos"
PAIR_LONGEST_FIRST, PAIR_ONLY_FIRST, PAIR_ONLY_SECOND, PAIR_MAX_SEP = 0, 1, 2, 4  # HUTK_PAIR_*
SPANS_BYTES, SPANS_CHARS = 0, 1
DECODE_SKIP_SPECIAL = 1  # HUTK_DECODE_SKIP_SPECIAL
FB_SPECIAL, FB_SKIP_SPECIAL = 1, 2  # HUTK_FB_*
NFC, NFD, NFKC, NFKD = 0, 1, 2, 3  # HUTK_NFC ..
MLM_SIDE_A, MLM_SIDE_B = 1, 2  # HUTK_MLM_SIDE_*
LABELS_A, LABELS_B, LABELS_TEMPLATE, LABELS_END, LABELS_SHIFT = 1, 2, 4, 8, 16  # HUTK_LABELS_*
CHAT_MAX_ROLES, CHAT_MAX_PART = 16, 32  # HUTK_CHAT_MAX_*
PACKER_MAX_CHANNELS = 4  # HUTK_PACKER_MAX_CHANNELS
FIM_PLAIN, FIM_PSM, FIM_SPM = 0, 1, 2  # HUTK_FIM_*: the kinds
WP_CLEAN_TEXT, WP_CJK, WP_STRIP_ACCENTS, WP_LOWERCASE = 1, 2, 4, 8  # HUTK_WP_*
FIM_PARTS = ("plain", "prefix", "middle", "suffix", "sentinel")  # HUTK_FIM_PART_*: a part's number is its index here

_lib = None


def library_path():
    return _build.LIB_HIP


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels carry their own copy of the HIP and HSA runtimes (torch/lib), and a process can
    open the GPU through ONE runtime only: with /opt/rocm's loaded first by this library, a later `import
    torch` finds "No HIP GPUs".  So when torch is installed but not yet imported, its copy is loaded here
    (by path, without importing torch); libhutoken_amd.so then binds to it by soname, and torch to the
    same file later.  HUTOKEN_AMD_SYSTEM_HIP=1 keeps /opt/rocm's."""
    if "torch" in sys.modules or os.environ.get("HUTOKEN_AMD_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load(build_if_missing=True):
    """Load libhutoken_amd.so (building it with hipcc when it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    # HUTOKEN_AMD_LIB: another build of the same library (tools/ab.py compares two on one GPU box)
    path = os.environ.get("HUTOKEN_AMD_LIB") or _build.LIB_HIP
    if path == _build.LIB_HIP and build_if_missing and (not os.path.exists(path) or os.environ.get("HUTOKEN_AMD_REBUILD")):
        _build.build_hip()
    if not os.path.exists(path):
        raise RuntimeError("hutoken_amd: native library %s is missing (run `python -m hutoken_amd.build`)" % path)
    L = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(L, name):  # (an older build under HUTOKEN_AMD_LIB, tools/ab.py, lacks the newer ones)
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


_shim = False


def shim():
    """The compiled CPython shim (csrc/pyshim/_hutoken_amd.c: the reference's _hutoken method table on this library), or
    None when it is not built or HUTOKEN_AMD_NO_SHIM is set.  Loaded after the library itself (see load())."""
    global _shim
    if _shim is False:
        _shim = None
        path = _build.LIB_PYSHIM
        if not os.environ.get("HUTOKEN_AMD_NO_SHIM") and not os.environ.get("HUTOKEN_AMD_LIB"):
            try:
                try:
                    _build.build_pyshim(force=bool(os.environ.get("HUTOKEN_AMD_REBUILD")))  # (checks for staleness itself)
                except Exception:
                    if not os.path.exists(path):  # no compiler and nothing built earlier
                        raise
                load()
                spec = importlib.util.spec_from_file_location("_hutoken_amd", path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                _shim = mod
            except Exception as e:  # no compiler, no Python.h: the ctypes path does the same work, 4x slower on lists
                import warnings
                warnings.warn("hutoken_amd: the compiled CPython shim is not available (%s); using ctypes" % (e,),
                              RuntimeWarning, stacklevel=2)
                _shim = None
    return _shim


def last_error():
    return load().hutk_last_error().decode("utf-8", "replace")


_EXC = {E_FILE_NOT_FOUND: FileNotFoundError, E_VALUE: ValueError, E_MEMORY: MemoryError,
        E_ARG: TypeError, E_DEVICE: RuntimeError, E_UNSUPPORTED: ValueError,
        E_CAPACITY: RuntimeError, E_NUL_BYTE: ValueError, E_WORD_TOO_LARGE: RuntimeError,
        E_INVALID_UTF8: ValueError}


def raise_for(code):
    if code != OK:
        raise _EXC.get(code, RuntimeError)(last_error())


class PinnedArray:
    """A numpy array on page-locked host memory from hutk_host_alloc (kept alive by this object)."""

    def __init__(self, n, dtype):
        import numpy as np
        self.dtype = np.dtype(dtype)
        self.nbytes = max(int(n) * self.dtype.itemsize, 1)
        self._p = load().hutk_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError("hutk_host_alloc failed")
        buf = (C.c_uint8 * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(n))

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            load().hutk_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Owner:
    """Owns one handle of the library (self._h) and gives it back through the function named by _destroy, unless somebody
    else owns it (_owned is False)."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                getattr(load(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Owner):
    """Owns one hutk_ctx."""
    _destroy = "hutk_ctx_destroy"

    def __init__(self, vocab_path, special_path, prefix=None, is_byte_encoder=False, device=-1, merges_path=None,
                 devices=None):
        """devices: several ordinals of this process; encode_packed() / hutk_encode_batch then spreads a large batch
        over them (hutk_ctx_add_device).  The first one is the context's own device."""
        L = load()
        if devices:
            device = int(devices[0])
        h = C.c_void_p()
        rc = L.hutk_ctx_create_merges(C.byref(h), os.fsencode(vocab_path), os.fsencode(special_path),
                                      None if prefix is None else prefix.encode("utf-8"),
                                      1 if is_byte_encoder else 0,
                                      None if merges_path is None else os.fsencode(merges_path), device)
        raise_for(rc)
        self._h = h
        self._owned = True
        for d in (devices or [])[1:]:
            try:
                self.add_device(int(d))
            except Exception:
                self.close()
                raise

    def add_device(self, device):
        raise_for(load().hutk_ctx_add_device(self._h, device))

    @property
    def device_count(self):
        return load().hutk_ctx_device_count(self._h)

    @classmethod
    def from_handle(cls, address):
        """A view of a hutk_ctx that somebody else owns (the CPython shim's module-global context)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(address)
        self._owned = False
        return self

    def set_pattern(self, pattern):
        """The regex pre-token path (initialize's `pattern`, a POSIX ERE); None: the hand-written splitter."""
        raise_for(load().hutk_ctx_set_pattern(self._h, None if pattern is None else pattern.encode("utf-8")))

    def set_pretokenizer(self, preset, blob=None):
        """A split preset (index into hutoken_amd.pretokenize.PRESETS) with its table blob; None: the built-in split."""
        if preset is None:
            raise_for(load().hutk_ctx_set_pretokenizer(self._h, -1, None, 0))
            return
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
        raise_for(load().hutk_ctx_set_pretokenizer(self._h, int(preset), C.cast(buf, C.c_void_p), len(blob)))

    @property
    def pretokenizer(self):
        """The installed preset's index, None: none."""
        p = load().hutk_ctx_pretokenizer(self._h)
        return None if p < 0 else p

    @property
    def uses_merges(self):
        """True when the id-keyed merge path (merges file) is in force."""
        return bool(load().hutk_uses_merges(self._h))

    @property
    def handle(self):
        return self._h

    def ids_capacity(self, n_bytes, n_docs):
        return load().hutk_ids_capacity(self._h, n_bytes, n_docs)

    def table_stats(self):
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_table_stats(self._h, out.ctypes.data))
        keys = ["n_keys", "n_vocab_sym", "n_sym", "n_pairs", "pair_slots", "rank_is_sym", "ident_ids", "n_word_entries"]
        d = dict(zip(keys, out.tolist()))
        if hasattr(load(), "hutk_debug_long_words"):
            d["n_long_word_entries"] = int(load().hutk_debug_long_words(self._h))
        return d

    def seam_map(self):
        """-> (uint32[256], in use): bit y - 0xE0 of entry x set = some merge can join input bytes x | y."""
        import numpy as np
        out = np.zeros(256, dtype=np.uint32)
        on = load().hutk_debug_seam(self._h, out.ctypes.data)
        return out, bool(on)

    def seam2_cut(self, a3, b3):
        """The seam map's second level: True when no token can span the three-byte characters a3 | b3 (bytes objects)."""
        return bool(load().hutk_debug_seam2_cut(self._h, int.from_bytes(a3, "little"), int.from_bytes(b3, "little")))

    def tile_kernel(self, n_bytes):
        """Which tile kernel hutk_encode_batch_device gives a plain batch of n_bytes under the environment of this moment:
        0 = k_tiles, 1 = k_ptiles (the persistent one), 2 = both, chosen on the device.  Launches nothing."""
        k = load().hutk_debug_tile_kernel(self._h, int(n_bytes))
        if k < 0:
            raise_for(E_ARG)
        return k

    def exc_counts(self):
        """Where the exception words of the most recent encode went (encode_device(), its stream synchronised by the
        caller, or a host form): {"exc": records, "lists": [up to 128 units, up to 256, up to 512, up to 1024, a wavefront
        each], "tail": 0 the full tail / 1 k_tail_small / 2 the one-launch k_tiles alone / 3 k_tail_small behind it,
        "has_multi": bool}.  One device-to-host copy, no launch."""
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_debug_exc_counts(self._h, out.ctypes.data))
        v = out.tolist()
        return {"exc": v[0], "lists": v[1:6], "tail": v[6], "has_multi": bool(v[7])}

    def word_cache_stats(self):
        """The learned table of multi-token words: {"entries", "capacity" (slots; 0: the context has no table), "appended":
        candidates the last learning batch handed to the table, "open": it still learns}.  Waits for the context's last call."""
        import numpy as np
        out = np.zeros(4, dtype=np.int64)
        raise_for(load().hutk_ctx_word_cache_stats(self._h, out.ctypes.data))
        v = out.tolist()
        return {"entries": v[0], "capacity": v[1], "appended": v[2], "open": bool(v[3])}

    def word_cache_clear(self):
        """Empty the learned table of multi-token words; it learns again from the next large batch."""
        raise_for(load().hutk_ctx_word_cache_clear(self._h))

    def _encode_host(self, fn, capacity, data, offsets, flags=()):
        """Host numpy buffers through the library's host encode `fn` (its flags, if it takes any, as a 1-tuple) with ids
        for capacity(n_bytes, n_docs).  -> (ids, out_offsets, status, return code); the caller judges the code."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        nbytes = int(offsets[n]) if n >= 0 else 0
        cap = capacity(nbytes, n)
        ids = np.empty(max(cap, 1), dtype=np.int32)
        oo = np.zeros(n + 1, dtype=np.int64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        rc = fn(self._h, data.ctypes.data if nbytes else None, offsets.ctypes.data, n, *flags, ids.ctypes.data, cap,
                oo.ctypes.data, st.ctypes.data)
        return ids[: int(oo[n])], oo, st[:n], rc

    def _decode_host(self, fn, ids, id_offsets, flags=()):
        """Host numpy buffers through the library's host decode `fn` (flags as in _encode_host), called twice: sizes,
        then the text.  -> (bytes, out_offsets, status)"""
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        id_offsets = np.ascontiguousarray(id_offsets, dtype=np.int64)
        n = len(id_offsets) - 1
        oo = np.zeros(n + 1, dtype=np.int64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        pid = ids.ctypes.data if len(ids) else None
        raise_for(fn(self._h, pid, id_offsets.ctypes.data, n, *flags, None, 0, oo.ctypes.data, st.ctypes.data))
        total = int(oo[n])
        out = np.empty(max(total, 1), dtype=np.uint8)
        raise_for(fn(self._h, pid, id_offsets.ctypes.data, n, *flags, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data))
        return out[:total], oo, st[:n]

    def encode_packed(self, data, offsets, want_status=True):
        """Host numpy buffers in, host numpy buffers out.
        -> (ids int32, out_offsets int64, status int32, return code)"""
        r = self._encode_host(load().hutk_encode_batch, self.ids_capacity, data, offsets)
        if r[3] not in (OK, E_WORD_TOO_LARGE):
            raise_for(r[3])
        return r

    def decode_packed(self, ids, id_offsets):
        """Decode direction, host numpy buffers: ids int32 + id_offsets int64[n+1] ->
        (bytes uint8, out_offsets int64[n+1], status int32[n]).  Two calls: sizes, then the text."""
        return self._decode_host(load().hutk_decode_batch, ids, id_offsets)

    def decode_device(self, d_ids, d_id_offsets, n_docs, n_ids, d_bytes_out, bytes_cap, d_out_offsets, d_status,
                      d_err, stream):
        """Raw device pointers (ints); asynchronous on `stream`."""
        raise_for(load().hutk_decode_batch_device(self._h, d_ids, d_id_offsets, n_docs, n_ids, d_bytes_out, bytes_cap,
                                                  d_out_offsets, d_status, d_err, stream))

    def encode_one(self, data: bytes):
        """-> (ids list, return code)"""
        import numpy as np
        L = load()
        n = len(data)
        cap = self.ids_capacity(n, 1)
        ids = np.empty(max(cap, 1), dtype=np.int32)
        n_ids = C.c_int64(0)
        st = C.c_int32(0)
        buf = C.create_string_buffer(data, n) if n else None
        rc = L.hutk_encode(self._h, C.cast(buf, C.c_void_p) if n else None, n, ids.ctypes.data, cap,
                           C.byref(n_ids), C.byref(st))
        if rc not in (OK, E_WORD_TOO_LARGE):
            raise_for(rc)
        return ids[: n_ids.value].tolist(), rc

    def encode_device(self, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets,
                      d_status=0, d_err=0, stream=0):
        """Raw device pointers (ints); asynchronous on `stream`."""
        rc = load().hutk_encode_batch_device(self._h, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap,
                                             d_out_offsets, d_status or None, d_err or None, stream or None)
        raise_for(rc)

    def token_spans_device(self, d_bytes, d_offsets, n_docs, n_bytes, d_ids, d_id_offsets, n_ids, unit, out_width,
                           d_spans, d_status=0, d_err=0, stream=0):
        """hutk_token_spans_device on raw device pointers (ints); asynchronous on `stream`."""
        raise_for(load().hutk_token_spans_device(self._h, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                 d_ids or None, d_id_offsets or None, n_ids, unit, out_width,
                                                 d_spans or None, d_status or None, d_err or None, stream or None))

    def token_spans_packed(self, data, offsets, ids, id_offsets, unit=SPANS_CHARS, out_width=4):
        """Host numpy buffers in and out (hutk_token_spans): -> (spans [n_ids, 2], status int32[n_docs], return code).
        A span mismatch (return code E_UNSUPPORTED) is reported through the status, anything else raises."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        id_offsets = np.ascontiguousarray(id_offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0 or len(id_offsets) != n + 1:
            raise TypeError("offsets and id_offsets must hold n_docs + 1 entries each")
        if n and (int(offsets[n]) > len(data) or int(id_offsets[n]) > len(ids)):
            raise TypeError("offsets point outside the buffers")
        n_ids = int(id_offsets[n])
        spans = np.zeros((n_ids, 2), dtype=np.int32 if out_width == 4 else np.int64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        rc = load().hutk_token_spans(self._h, data.ctypes.data if len(data) else None, offsets.ctypes.data, n,
                                     ids.ctypes.data if len(ids) else None, id_offsets.ctypes.data, unit, out_width,
                                     spans.ctypes.data if n_ids else None, st.ctypes.data)
        if rc != OK and not (rc == E_UNSUPPORTED and (st[:n] == DOC_SPAN_MISMATCH).any()):
            raise_for(rc)
        return spans, st[:n], rc

    def set_special_tokens(self, pairs):
        """Install special tokens (hutk_ctx_set_special_tokens): `pairs` is a sequence of (bytes, id); an empty one
        removes the set.  ValueError for a set the library refuses."""
        import numpy as np
        pairs = list(pairs)
        n = len(pairs)
        if n == 0:
            raise_for(load().hutk_ctx_set_special_tokens(self._h, None, None, None, 0))
            return
        blob = b"".join(bytes(k) for k, _i in pairs)
        data = np.frombuffer(blob + b"\0", dtype=np.uint8)  # (never empty: an empty string is the library's to refuse)
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(k) for k, _i in pairs], out=offs[1:])
        for _k, i in pairs:
            if not -2**31 <= int(i) < 2**31:
                raise ValueError("the id of a special token must fit an int32")
        ids = np.array([int(i) for _k, i in pairs], dtype=np.int32)
        raise_for(load().hutk_ctx_set_special_tokens(self._h, data.ctypes.data, offs.ctypes.data, ids.ctypes.data, n))

    @property
    def special_token_count(self):
        return int(load().hutk_ctx_special_token_count(self._h))

    @property
    def special_last_matches(self):
        """Matches the last encode_special_* call on this context found."""
        return int(load().hutk_special_last_matches(self._h))

    def special_ids_capacity(self, n_bytes, n_docs):
        return load().hutk_special_ids_capacity(self._h, n_bytes, n_docs)

    def encode_special_packed(self, data, offsets):
        """encode_packed with the context's special tokens (hutk_encode_special_batch): host numpy buffers in and out.
        -> (ids int32, out_offsets int64, status int32, return code)"""
        r = self._encode_host(load().hutk_encode_special_batch, self.special_ids_capacity, data, offsets)
        if r[3] not in (OK, E_WORD_TOO_LARGE):
            raise_for(r[3])
        return r

    def encode_special_device(self, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets,
                              d_status=0, d_err=0, stream=0):
        """hutk_encode_special_batch_device on raw device pointers (ints): synchronises `stream` once, after the scan."""
        raise_for(load().hutk_encode_special_batch_device(self._h, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                          d_ids or None, ids_cap, d_out_offsets or None,
                                                          d_status or None, d_err or None, stream or None))

    def decode_special_packed(self, ids, id_offsets, flags=0):
        """decode_packed with the context's special tokens (hutk_decode_special_batch; flags: 0 or DECODE_SKIP_SPECIAL):
        -> (bytes uint8, out_offsets int64[n+1], status int32[n]).  Two calls: sizes, then the text."""
        return self._decode_host(load().hutk_decode_special_batch, ids, id_offsets, (flags,))

    def decode_special_device(self, d_ids, d_id_offsets, n_docs, n_ids, flags, d_bytes_out, bytes_cap, d_out_offsets,
                              d_status=0, d_err=0, stream=0):
        """hutk_decode_special_batch_device on raw device pointers (ints); asynchronous on `stream`, never synchronises."""
        raise_for(load().hutk_decode_special_batch_device(self._h, d_ids or None, d_id_offsets or None, n_docs, n_ids,
                                                          flags, d_bytes_out or None, bytes_cap, d_out_offsets or None,
                                                          d_status or None, d_err or None, stream or None))

    def find_byte_tokens(self):
        """-> (int32[256], found): the ids of the vocabulary keys "<0x00>".."<0xFF>", -1 where there is none."""
        import numpy as np
        out = np.zeros(256, dtype=np.int32)
        found = load().hutk_ctx_find_byte_tokens(self._h, out.ctypes.data)
        return out, int(found)

    def set_byte_fallback(self, ids256):
        """Install the byte-fallback table (hutk_ctx_set_byte_fallback): 256 ids, or None to remove it.  ValueError for a
        table the library refuses."""
        import numpy as np
        if ids256 is None:
            raise_for(load().hutk_ctx_set_byte_fallback(self._h, None))
            return
        ids = [int(i) for i in ids256]
        if len(ids) != 256:
            raise ValueError("a byte-fallback table holds 256 ids")
        if any(not -2**31 <= i < 2**31 for i in ids):
            raise ValueError("the ids of a byte-fallback table must fit an int32")
        arr = np.array(ids, dtype=np.int32)
        raise_for(load().hutk_ctx_set_byte_fallback(self._h, arr.ctypes.data))

    @property
    def byte_fallback(self):
        """The installed table (int32[256]) or None."""
        import numpy as np
        out = np.zeros(256, dtype=np.int32)
        return out if load().hutk_ctx_byte_fallback(self._h, out.ctypes.data) else None

    def encode_fallback_packed(self, data, offsets, flags=0):
        """encode_packed with byte fallback (hutk_encode_fallback_batch; flags: 0 or FB_SPECIAL): host numpy buffers in
        and out.  -> (ids int32, out_offsets int64, status int32, return code); the code E_UNSUPPORTED (documents whose
        spans did not verify keep their plain ids) is returned, not raised."""
        capacity = self.special_ids_capacity if flags & FB_SPECIAL else self.ids_capacity
        r = self._encode_host(load().hutk_encode_fallback_batch, capacity, data, offsets, (flags,))
        if r[3] not in (OK, E_WORD_TOO_LARGE) and not (r[3] == E_UNSUPPORTED and len(r[0]) > 0):
            raise_for(r[3])
        return r

    def encode_fallback_device(self, d_bytes, d_offsets, n_docs, n_bytes, flags, d_ids, ids_cap, d_out_offsets,
                               d_status=0, d_err=0, stream=0):
        """hutk_encode_fallback_batch_device on raw device pointers (ints); asynchronous on `stream` (with FB_SPECIAL it
        synchronises once, as the special encode does)."""
        raise_for(load().hutk_encode_fallback_batch_device(self._h, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                           flags, d_ids or None, ids_cap, d_out_offsets or None,
                                                           d_status or None, d_err or None, stream or None))

    def decode_fallback_packed(self, ids, id_offsets, flags=0):
        """decode_packed with byte fallback (hutk_decode_fallback_batch; flags: FB_SPECIAL, FB_SKIP_SPECIAL):
        -> (bytes uint8, out_offsets int64[n+1], status int32[n]).  Two calls: sizes, then the text."""
        return self._decode_host(load().hutk_decode_fallback_batch, ids, id_offsets, (flags,))

    def decode_fallback_device(self, d_ids, d_id_offsets, n_docs, n_ids, flags, d_bytes_out, bytes_cap, d_out_offsets,
                               d_status=0, d_err=0, stream=0):
        """hutk_decode_fallback_batch_device on raw device pointers (ints); asynchronous on `stream`, never synchronises."""
        raise_for(load().hutk_decode_fallback_batch_device(self._h, d_ids or None, d_id_offsets or None, n_docs, n_ids,
                                                           flags, d_bytes_out or None, bytes_cap, d_out_offsets or None,
                                                           d_status or None, d_err or None, stream or None))

    def profile(self, enable):
        load().hutk_debug_profile(self._h, 1 if enable else 0)

    def profile_read(self, n_tiles):
        import numpy as np
        out = np.zeros(10, dtype=np.float64)
        raise_for(load().hutk_debug_profile_read(self._h, n_tiles, out.ctypes.data))
        return out.tolist()

    def profile_raw(self, n_tiles):
        import numpy as np
        out = np.zeros((n_tiles, 10), dtype=np.int64)
        raise_for(load().hutk_debug_profile_raw(self._h, n_tiles, out.ctypes.data))
        return out

    def last_timing(self):
        a, b = C.c_float(0), C.c_float(0)
        raise_for(load().hutk_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


TRAINER_STATS = ["docs", "bytes", "word_occurrences", "unique_words", "symbols", "pairs_at_start",
                 "peak_device_bytes", "merge_loop_us"]
# hutk_trainer_debug_counters, in its order
TRAINER_COUNTERS = ["pauses", "pair_grows", "pair_shrinks", "pair_rebuilds", "host_syncs", "pair_cap_max",
                    "select_blocks_max", "word_rehashes", "deferred_words", "insert_rounds_max", "long_to_short",
                    "dropped_words", "charset_grows"]


class Trainer(_Owner):
    """Owns one hutk_trainer (BPE training on the GPU, include/hutoken_amd.h); mode TRAIN_BYTES or TRAIN_CHARS."""
    _destroy = "hutk_trainer_destroy"

    def __init__(self, device=-1, mode=TRAIN_BYTES):
        h = C.c_void_p()
        raise_for(load().hutk_trainer_create_mode(C.byref(h), int(device), int(mode)))
        self._h = h

    def alphabet(self):
        """The initial symbols in id order (list of bytes); ends the adding phase."""
        import numpy as np
        n_sym, n_bytes = C.c_int64(0), C.c_int64(0)
        raise_for(load().hutk_trainer_alphabet(self._h, None, 0, None, 0, C.byref(n_sym), C.byref(n_bytes)))
        data = np.zeros(max(n_bytes.value, 1), dtype=np.uint8)
        offs = np.zeros(n_sym.value + 1, dtype=np.int64)
        raise_for(load().hutk_trainer_alphabet(self._h, data.ctypes.data, len(data), offs.ctypes.data, len(offs),
                                               C.byref(n_sym), C.byref(n_bytes)))
        raw = data.tobytes()
        return [raw[offs[i]:offs[i + 1]] for i in range(n_sym.value)]

    def add_packed(self, data, offsets):
        """Packed bytes (uint8) + int64 offsets[n+1]: documents data[offsets[i]:offsets[i+1]]."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0:
            raise ValueError("offsets must hold at least one entry")
        if n and (int(offsets[0]) < 0 or int(offsets[n]) > len(data)):
            raise ValueError("offsets point outside data")
        raise_for(load().hutk_trainer_add(self._h, data.ctypes.data if len(data) else None, offsets.ctypes.data, n))

    def run(self, n_merges):
        """-> (pairs int32[m, 2], counts int64[m]), m <= n_merges."""
        import numpy as np
        n_merges = int(n_merges)
        if n_merges > 2**31 - 1:  # (the C ABI takes an int32_t; ctypes would truncate silently)
            raise ValueError("n_merges must be at most 2**31 - 1")
        if n_merges > 0:  # every merge removes a symbol: the C side never does more than the corpus holds
            n_merges = min(n_merges, self.stats()["symbols"])
        pairs = np.zeros((max(n_merges, 1), 2), dtype=np.int32)
        counts = np.zeros(max(n_merges, 1), dtype=np.int64)
        done = C.c_int32(0)
        raise_for(load().hutk_trainer_run(self._h, n_merges, pairs.ctypes.data, counts.ctypes.data, C.byref(done)))
        return pairs[:done.value].copy(), counts[:done.value].copy()

    def stats(self):
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_trainer_stats(self._h, out.ctypes.data))
        return dict(zip(TRAINER_STATS, out.tolist()))

    def debug_counters(self):
        """Which internal paths add() and run() took (include/hutoken_amd.h, hutk_trainer_debug_counters)."""
        import numpy as np
        out = np.zeros(len(TRAINER_COUNTERS), dtype=np.int64)
        raise_for(load().hutk_trainer_debug_counters(self._h, out.ctypes.data, len(out)))
        return dict(zip(TRAINER_COUNTERS, out.tolist()))


def collate_padded_device(d_ids, d_offsets, n_docs, n_ids, max_len, bos_id, eos_id, pad_id, flags, out_width,
                          d_input_ids, d_mask=0, d_lengths=0, d_err=0, stream=0):
    """hutk_collate_padded_device on raw device pointers (ints); asynchronous on `stream`.  bos_id / eos_id: NO_TOKEN
    when absent."""
    raise_for(load().hutk_collate_padded_device(d_ids or None, d_offsets or None, n_docs, n_ids, max_len, bos_id,
                                                eos_id, pad_id, flags, out_width, d_input_ids or None,
                                                d_mask or None, d_lengths or None, d_err or None, stream or None))


def windows_rows_bound(n_docs, n_ids, max_len, stride, s):
    """hutk_windows_rows_bound (host only): an upper bound of the rows collate_windows_device writes."""
    n = load().hutk_windows_rows_bound(n_docs, n_ids, max_len, stride, s)
    if n < 0:
        raise_for(-n)
    return n


def windows_rows_device(d_offsets, n_docs, n_ids, max_len, stride, bos_id, eos_id, d_row_offsets, d_err=0, stream=0):
    """hutk_windows_rows_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_windows_rows_device(d_offsets or None, n_docs, n_ids, max_len, stride, bos_id, eos_id,
                                              d_row_offsets or None, d_err or None, stream or None))


def collate_windows_device(d_ids, d_offsets, d_row_offsets, n_docs, n_ids, n_rows, max_len, stride, bos_id, eos_id,
                           pad_id, flags, out_width, d_input_ids, d_mask=0, d_lengths=0, d_row_map=0, d_err=0, stream=0):
    """hutk_collate_windows_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_collate_windows_device(d_ids or None, d_offsets or None, d_row_offsets or None, n_docs, n_ids,
                                                 n_rows, max_len, stride, bos_id, eos_id, pad_id, flags, out_width,
                                                 d_input_ids or None, d_mask or None, d_lengths or None,
                                                 d_row_map or None, d_err or None, stream or None))


def _sep_array(sep_ids):
    """tuple of ints -> (a ctypes int32 array the call may read, its length); the C ABI checks the values."""
    sep_ids = tuple(sep_ids)
    return (_s32 * max(1, len(sep_ids)))(*sep_ids), len(sep_ids)


def pair_rows_bound(n_pairs, n_cut_ids, max_len, stride, s):
    """hutk_pair_rows_bound (host only): an upper bound of the rows the windows form of collate_pairs_device writes."""
    n = load().hutk_pair_rows_bound(n_pairs, n_cut_ids, max_len, stride, s)
    if n < 0:
        raise_for(-n)
    return n


def pair_rows_device(d_offsets_a, d_offsets_b, n_pairs, cap_a, cap_b, max_len, stride, strategy, bos_id, sep_ids, eos_id,
                     d_row_offsets, d_err=0, stream=0):
    """hutk_pair_rows_device on raw device pointers (ints); sep_ids: a tuple of ints; asynchronous on `stream`."""
    sep, n_sep = _sep_array(sep_ids)
    raise_for(load().hutk_pair_rows_device(d_offsets_a or None, d_offsets_b or None, n_pairs, cap_a, cap_b, max_len, stride,
                                           strategy, bos_id, sep, n_sep, eos_id, d_row_offsets or None, d_err or None,
                                           stream or None))


def collate_pairs_device(d_ids_a, d_offsets_a, d_ids_b, d_offsets_b, d_row_offsets, n_pairs, cap_a, cap_b, n_rows, max_len,
                         stride, strategy, bos_id, sep_ids, eos_id, pad_id, flags, out_width, d_input_ids, d_mask=0,
                         d_token_types=0, d_lengths=0, d_row_map=0, d_err=0, stream=0):
    """hutk_collate_pairs_device on raw device pointers (ints); d_row_offsets 0: one row per pair; sep_ids: a tuple of
    ints; asynchronous on `stream`."""
    sep, n_sep = _sep_array(sep_ids)
    raise_for(load().hutk_collate_pairs_device(d_ids_a or None, d_offsets_a or None, d_ids_b or None, d_offsets_b or None,
                                               d_row_offsets or None, n_pairs, cap_a, cap_b, n_rows, max_len, stride,
                                               strategy, bos_id, sep, n_sep, eos_id, pad_id, flags, out_width,
                                               d_input_ids or None, d_mask or None, d_token_types or None,
                                               d_lengths or None, d_row_map or None, d_err or None, stream or None))


def padded_plan_device(d_offsets, n_docs, n_ids, max_len, bos_id, eos_id, flags, d_plan, d_err=0, stream=0):
    """hutk_padded_plan_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_padded_plan_device(d_offsets or None, n_docs, n_ids, max_len, bos_id, eos_id, flags,
                                             d_plan or None, d_err or None, stream or None))


def windows_plan_device(d_offsets, d_row_offsets, n_docs, n_ids, n_rows, max_len, stride, bos_id, eos_id, flags, d_plan,
                        d_err=0, stream=0):
    """hutk_windows_plan_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_windows_plan_device(d_offsets or None, d_row_offsets or None, n_docs, n_ids, n_rows, max_len,
                                              stride, bos_id, eos_id, flags, d_plan or None, d_err or None, stream or None))


def pair_plan_device(d_offsets_a, d_offsets_b, d_row_offsets, n_pairs, cap_a, cap_b, n_rows, max_len, stride, strategy,
                     bos_id, sep_ids, eos_id, flags, d_plan, d_err=0, stream=0):
    """hutk_pair_plan_device on raw device pointers (ints); d_row_offsets 0: one row per pair; sep_ids: a tuple of ints;
    asynchronous on `stream`."""
    sep, n_sep = _sep_array(sep_ids)
    raise_for(load().hutk_pair_plan_device(d_offsets_a or None, d_offsets_b or None, d_row_offsets or None, n_pairs, cap_a,
                                           cap_b, n_rows, max_len, stride, strategy, bos_id, sep, n_sep, eos_id, flags,
                                           d_plan or None, d_err or None, stream or None))


def rows_gather_device(d_plan, n_rows, max_len, d_values_a, n_a, d_values_b, n_b, rec_bytes, fill, d_out, d_err=0, stream=0):
    """hutk_rows_gather_device on raw device pointers (ints); fill: the record as bytes of length rec_bytes;
    asynchronous on `stream`."""
    buf = (C.c_uint8 * 16).from_buffer_copy(bytes(fill).ljust(16, b"\0"))
    raise_for(load().hutk_rows_gather_device(d_plan or None, n_rows, max_len, d_values_a or None, n_a, d_values_b or None,
                                             n_b, rec_bytes, C.cast(buf, C.c_void_p), d_out or None, d_err or None,
                                             stream or None))


def token_word_ids_device(d_word_bits, d_before, d_offsets, n_docs, n_bytes, d_spans, span_width, d_id_offsets, n_ids,
                          d_word_ids, d_status=0, d_err=0, stream=0):
    """hutk_token_word_ids_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_token_word_ids_device(d_word_bits or None, d_before or None, d_offsets or None, n_docs, n_bytes,
                                                d_spans or None, span_width, d_id_offsets or None, n_ids,
                                                d_word_ids or None, d_status or None, d_err or None, stream or None))


def word_ids_tile():
    return load().hutk_debug_word_ids_tile()


def rows_answers_device(d_plan, n_rows, side, d_spans, span_width, n_spans, d_answers, n_items, d_out, d_err=0, stream=0):
    """hutk_rows_answers_device on raw device pointers (ints); side: 0 for A, 1 for B; asynchronous on `stream`."""
    raise_for(load().hutk_rows_answers_device(d_plan or None, n_rows, side, d_spans or None, span_width, n_spans,
                                              d_answers or None, n_items, d_out or None, d_err or None, stream or None))


def rows_mlm_device(d_plan, n_rows, max_len, d_input_ids, width, d_words_a, n_a, d_words_b, n_b, seed, select_below,
                    mask_below, random_below, mask_id, vocab_size, ignore_index, sides, d_out_ids, d_labels, d_err=0, stream=0):
    """hutk_rows_mlm_device on raw device pointers (ints); d_words_a == 0: token mode; the thresholds are ints in
    0 .. 2**32; asynchronous on `stream`."""
    raise_for(load().hutk_rows_mlm_device(d_plan or None, n_rows, max_len, d_input_ids or None, width, d_words_a or None, n_a,
                                          d_words_b or None, n_b, seed, select_below, mask_below, random_below, mask_id,
                                          vocab_size, ignore_index, sides, d_out_ids or None, d_labels or None,
                                          d_err or None, stream or None))


def rows_labels_device(d_plan, n_rows, max_len, d_input_ids, width, d_mask, flags, ignore_index, d_labels, d_err=0, stream=0):
    """hutk_rows_labels_device on raw device pointers (ints); flags: LABELS_*; asynchronous on `stream`."""
    raise_for(load().hutk_rows_labels_device(d_plan or None, n_rows, max_len, d_input_ids or None, width, d_mask or None,
                                             flags, ignore_index, d_labels or None, d_err or None, stream or None))


def rows_span_corrupt_device(d_plan, n_rows, max_len, d_input_ids, width, d_mask, seed, start_below, len_below, sentinel_first,
                             sentinel_step, n_sentinels, target_eos_id, decoder_start_id, pad_id, ignore_index, sides,
                             max_target_len, d_out_ids, d_out_mask, d_labels, d_decoder_ids, d_in_lengths, d_tgt_lengths,
                             d_err=0, stream=0):
    """hutk_rows_span_corrupt_device on raw device pointers (ints); len_below: a sequence of ints in 0 .. 2**32, the host
    table; target_eos_id / decoder_start_id: NO_TOKEN for none; asynchronous on `stream`."""
    table = (_i64 * len(len_below))(*len_below)
    raise_for(load().hutk_rows_span_corrupt_device(d_plan or None, n_rows, max_len, d_input_ids or None, width, d_mask or None,
                                                   seed, start_below, table, len(len_below), sentinel_first, sentinel_step,
                                                   n_sentinels, target_eos_id, decoder_start_id, pad_id, ignore_index, sides,
                                                   max_target_len, d_out_ids or None, d_out_mask or None, d_labels or None,
                                                   d_decoder_ids or None, d_in_lengths or None, d_tgt_lengths or None,
                                                   d_err or None, stream or None))


class Packer(_Owner):
    """Owns one hutk_packer (include/hutoken_amd.h): raw device pointers (ints) in, rows written asynchronously."""
    _destroy = "hutk_packer_destroy"

    def __init__(self, seq_len, bos_id=NO_TOKEN, eos_id=NO_TOKEN, pad_id=0, out_width=4, device=-1, channels=()):
        """channels: (width, per, fill) of each per-token array the packer moves with the ids (hutk_packer_create_channels;
        the C ABI checks them)."""
        h = C.c_void_p()
        channels = [tuple(c) for c in channels]
        if channels:
            n = len(channels)
            raise_for(load().hutk_packer_create_channels(
                C.byref(h), int(seq_len), int(bos_id), int(eos_id), int(pad_id), int(out_width), int(device), n,
                (C.c_int * n)(*(c[0] for c in channels)), (C.c_int * n)(*(c[1] for c in channels)),
                (_i64 * n)(*(c[2] for c in channels))))
        else:
            raise_for(load().hutk_packer_create(C.byref(h), int(seq_len), int(bos_id), int(eos_id), int(pad_id),
                                                int(out_width), int(device)))
        self._h = h

    @property
    def channel_count(self):
        return load().hutk_packer_channel_count(self._h)

    def add_channels(self, d_ids, d_offsets, n_docs, n_ids, d_values, d_input_ids, d_position_ids, d_segment_ids,
                     d_channel_rows, rows_cap, d_err=0, stream=0):
        """hutk_packer_add_channels_device: d_values / d_channel_rows are sequences of device pointers (ints), one per
        channel -> the number of rows written."""
        n = C.c_int64(0)
        raise_for(load().hutk_packer_add_channels_device(self._h, d_ids or None, d_offsets or None, n_docs, n_ids,
                                                         _pointer_array(d_values), d_input_ids or None, d_position_ids or None,
                                                         d_segment_ids or None, _pointer_array(d_channel_rows), rows_cap,
                                                         C.byref(n), d_err or None, stream or None))
        return n.value

    def flush_channels(self, d_input_ids, d_position_ids, d_segment_ids, d_channel_rows, stream=0):
        """hutk_packer_flush_channels_device -> 0 or 1 rows written."""
        n = C.c_int64(0)
        raise_for(load().hutk_packer_flush_channels_device(self._h, d_input_ids or None, d_position_ids or None,
                                                           d_segment_ids or None, _pointer_array(d_channel_rows), C.byref(n),
                                                           stream or None))
        return n.value

    def rows(self, n_docs, n_ids):
        """Rows the next add() with these sizes writes."""
        return load().hutk_packer_rows(self._h, n_docs, n_ids)

    @property
    def pending(self):
        return load().hutk_packer_pending(self._h)

    def add(self, d_ids, d_offsets, n_docs, n_ids, d_input_ids, d_position_ids, d_segment_ids, rows_cap, d_err=0,
            stream=0):
        """-> the number of rows written."""
        n = C.c_int64(0)
        raise_for(load().hutk_packer_add_device(self._h, d_ids or None, d_offsets or None, n_docs, n_ids,
                                                d_input_ids or None, d_position_ids or None, d_segment_ids or None,
                                                rows_cap, C.byref(n), d_err or None, stream or None))
        return n.value

    def flush(self, d_input_ids, d_position_ids, d_segment_ids, stream=0):
        """-> 0 or 1 rows written."""
        n = C.c_int64(0)
        raise_for(load().hutk_packer_flush_device(self._h, d_input_ids or None, d_position_ids or None,
                                                  d_segment_ids or None, C.byref(n), stream or None))
        return n.value


def _pointer_array(pointers):
    """device pointers (ints; 0: NULL) -> a host array of them the call may read, or NULL for an empty sequence"""
    pointers = tuple(pointers)
    return (_vp * len(pointers))(*(p or None for p in pointers)) if pointers else None


def packed_cu_seqlens_device(d_segment_ids, n_rows, seq_len, cap, d_cu_seqlens, d_info, d_err=0, stream=0):
    """hutk_packed_cu_seqlens_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_packed_cu_seqlens_device(d_segment_ids or None, n_rows, seq_len, cap, d_cu_seqlens or None,
                                                   d_info or None, d_err or None, stream or None))


def packed_labels_device(d_values, width, d_segment_ids, n_rows, seq_len, shift, ignore_index, d_labels, stream=0):
    """hutk_packed_labels_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_packed_labels_device(d_values or None, width, d_segment_ids or None, n_rows, seq_len,
                                               1 if shift else 0, ignore_index, d_labels or None, stream or None))


def cu_tile():
    return load().hutk_debug_cu_tile()


def bestfit_rows_bound(n_docs, n_ids, seq_len, s):
    """hutk_bestfit_rows_bound (host only): an upper bound of the rows best-fit packing gives."""
    n = load().hutk_bestfit_rows_bound(n_docs, n_ids, seq_len, s)
    if n < 0:
        raise_for(-n)
    return n


def bestfit_plan_device(d_offsets, n_docs, n_ids, seq_len, bos_id, eos_id, rows_cap, d_doc_map, d_info, d_err=0, stream=0):
    """hutk_bestfit_plan_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_bestfit_plan_device(d_offsets or None, n_docs, n_ids, seq_len, bos_id, eos_id, rows_cap,
                                              d_doc_map or None, d_info or None, d_err or None, stream or None))


def bestfit_rows_device(d_ids, d_offsets, d_doc_map, n_docs, n_ids, seq_len, bos_id, eos_id, pad_id, out_width, rows_cap,
                        d_input_ids, d_position_ids, d_segment_ids, d_lengths, d_source=0, d_err=0, stream=0):
    """hutk_bestfit_rows_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_bestfit_rows_device(d_ids or None, d_offsets or None, d_doc_map or None, n_docs, n_ids, seq_len,
                                              bos_id, eos_id, pad_id, out_width, rows_cap, d_input_ids or None,
                                              d_position_ids or None, d_segment_ids or None, d_lengths or None,
                                              d_source or None, d_err or None, stream or None))


def rows_gather_source_device(d_source, n, d_values, n_values, width, per, fill, d_out, d_err=0, stream=0):
    """hutk_rows_gather_source_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_rows_gather_source_device(d_source or None, n, d_values or None, n_values, width, per, fill,
                                                    d_out or None, d_err or None, stream or None))


def bestfit_tile():
    return load().hutk_debug_bestfit_tile()


def _i32_array(values):
    """ints -> a ctypes int32 array the call may read (never of length 0); the C ABI checks the values."""
    values = tuple(values)
    return (_s32 * max(1, len(values)))(*values)


class ChatTemplate(_Owner):
    """Owns one hutk_chat_template (include/hutoken_amd.h): parts = [(prefix ids, suffix ids)] per role, suffix_loss a
    list of ints or None, bos_id / eos_id NO_TOKEN when absent.  The ids must fit an int32 (the caller's check)."""
    _destroy = "hutk_chat_template_destroy"

    def __init__(self, parts, suffix_loss=None, bos_id=NO_TOKEN, eos_id=NO_TOKEN, device=-1, n_roles=None):
        parts = [(tuple(p), tuple(s)) for p, s in parts]
        pre, suf, po, so = [], [], [0], [0]
        for p, s in parts:
            pre += p
            suf += s
            po.append(len(pre))
            so.append(len(suf))
        h = C.c_void_p()
        raise_for(load().hutk_chat_template_create(C.byref(h), int(device), len(parts) if n_roles is None else n_roles,
                                                   _i32_array(pre), _i32_array(po), _i32_array(suf), _i32_array(so),
                                                   None if suffix_loss is None else _i32_array(suffix_loss),
                                                   int(bos_id), int(eos_id)))
        self._h = h

    def ids_bound(self, n_conv, n_turns, n_ids, gen_role=-1):
        """hutk_chat_ids_bound (host only): an upper bound of the ids a render of these sizes writes."""
        n = load().hutk_chat_ids_bound(self._h, n_conv, n_turns, n_ids, gen_role)
        if n < 0:
            raise_for(-n)
        return n

    def offsets_device(self, d_offsets, d_roles, d_conv_offsets, n_conv, n_turns, n_ids, gen_role, d_turn_offsets,
                       d_out_offsets, d_err=0, stream=0):
        """hutk_chat_offsets_device on raw device pointers (ints); asynchronous on `stream`."""
        raise_for(load().hutk_chat_offsets_device(self._h, d_offsets or None, d_roles or None, d_conv_offsets or None, n_conv,
                                                  n_turns, n_ids, gen_role, d_turn_offsets or None, d_out_offsets or None,
                                                  d_err or None, stream or None))

    def render_device(self, d_ids, d_offsets, d_roles, d_conv_offsets, d_turn_offsets, d_out_offsets, n_conv, n_turns, n_ids,
                      gen_role, loss_roles, ignore_index, out_cap, d_out_ids, d_labels, d_turn_ids=0, d_src=0, d_err=0,
                      stream=0):
        """hutk_chat_render_device on raw device pointers (ints); asynchronous on `stream`."""
        raise_for(load().hutk_chat_render_device(self._h, d_ids or None, d_offsets or None, d_roles or None,
                                                 d_conv_offsets or None, d_turn_offsets or None, d_out_offsets or None,
                                                 n_conv, n_turns, n_ids, gen_role, loss_roles, ignore_index, out_cap,
                                                 d_out_ids or None, d_labels or None, d_turn_ids or None, d_src or None,
                                                 d_err or None, stream or None))


def chat_span():
    return load().hutk_debug_chat_span()


def fim_ids_bound(n_docs, n_ids, has_end):
    """hutk_fim_ids_bound (host only): an upper bound of the ids a fill-in-the-middle render of these sizes writes."""
    n = load().hutk_fim_ids_bound(n_docs, n_ids, 1 if has_end else 0)
    if n < 0:
        raise_for(-n)
    return n


def fim_cut_text_device(d_bytes, d_offsets, n_docs, n_bytes, seed, first_doc, fim_below, spm_below, d_piece_offsets, d_kinds,
                        d_err=0, stream=0):
    """hutk_fim_cut_text_device on raw device pointers (ints); the thresholds are ints in 0 .. 2**32; asynchronous on
    `stream`."""
    raise_for(load().hutk_fim_cut_text_device(d_bytes or None, d_offsets or None, n_docs, n_bytes, seed, first_doc, fim_below,
                                              spm_below, d_piece_offsets or None, d_kinds or None, d_err or None,
                                              stream or None))


def fim_plan_tokens_device(d_offsets, n_docs, n_ids, seed, first_doc, fim_below, spm_below, has_end, d_out_offsets, d_plan,
                           d_kinds, d_err=0, stream=0):
    """hutk_fim_plan_tokens_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_fim_plan_tokens_device(d_offsets or None, n_docs, n_ids, seed, first_doc, fim_below, spm_below,
                                                 1 if has_end else 0, d_out_offsets or None, d_plan or None, d_kinds or None,
                                                 d_err or None, stream or None))


def fim_plan_pieces_device(d_piece_id_offsets, d_kinds, n_docs, n_ids, has_end, d_out_offsets, d_plan, d_err=0, stream=0):
    """hutk_fim_plan_pieces_device on raw device pointers (ints); asynchronous on `stream`."""
    raise_for(load().hutk_fim_plan_pieces_device(d_piece_id_offsets or None, d_kinds or None, n_docs, n_ids,
                                                 1 if has_end else 0, d_out_offsets or None, d_plan or None, d_err or None,
                                                 stream or None))


def fim_render_device(d_ids, d_plan, d_kinds, d_out_offsets, n_docs, n_ids, pre_id, suf_id, mid_id, end_id, loss_parts,
                      ignore_index, out_cap, d_out_ids, d_labels=0, d_parts=0, d_src=0, d_err=0, stream=0):
    """hutk_fim_render_device on raw device pointers (ints); end_id NO_TOKEN: none; asynchronous on `stream`."""
    raise_for(load().hutk_fim_render_device(d_ids or None, d_plan or None, d_kinds or None, d_out_offsets or None, n_docs,
                                            n_ids, pre_id, suf_id, mid_id, end_id, loss_parts, ignore_index, out_cap,
                                            d_out_ids or None, d_labels or None, d_parts or None, d_src or None,
                                            d_err or None, stream or None))


def fim_span():
    return load().hutk_debug_fim_span()


def fim_decide(seed, doc, length, fim_below, spm_below):
    """hutk_debug_fim_decide (host only) -> (kind, lo, hi)"""
    out = (_i64 * 3)()
    raise_for(load().hutk_debug_fim_decide(seed, doc, length, fim_below, spm_below, out))
    return out[0], out[1], out[2]


def fim_locate(n, lo, hi, kind, has_end, p):
    """hutk_debug_fim_locate (host only) -> (part, index inside the document or the sentinel's number)"""
    out = (_i64 * 2)()
    raise_for(load().hutk_debug_fim_locate(n, lo, hi, kind, 1 if has_end else 0, p, out))
    return out[0], out[1]


NORMALIZER_INFO = ["format_version", "unidata", "blob_bytes", "chunk_bytes", "pairs", "decomposition_words", "lead_bytes",
                   "max_expansion"]


class Normalizer(_Owner):
    """Owns one hutk_normalizer (Unicode normalisation on the GPU, include/hutoken_amd.h): the table blob of
    hutoken_amd.normalize on one device, and the workspace of its calls."""
    _destroy = "hutk_normalizer_destroy"

    def __init__(self, blob, device=-1):
        h = C.c_void_p()
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
        raise_for(load().hutk_normalizer_create(C.byref(h), int(device), C.cast(buf, C.c_void_p), len(blob)))
        self._h = h

    def info(self):
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_normalizer_info(self._h, out.ctypes.data))
        d = dict(zip(NORMALIZER_INFO, out.tolist()))
        for k in ("lead_bytes", "max_expansion"):
            d[k] = [(d[k] >> (8 * f)) & 0xFF for f in range(4)]
        return d

    def batch_device(self, form, d_bytes, d_offsets, n_docs, n_bytes, d_out, out_cap, d_out_offsets, d_changed=0,
                     d_totals=0, d_err=0, stream=0):
        """hutk_normalize_batch_device on raw device pointers (ints); d_out == 0: the sizes call.  Asynchronous on
        `stream`, never synchronises."""
        raise_for(load().hutk_normalize_batch_device(self._h, form, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                     d_out or None, out_cap, d_out_offsets or None, d_changed or None,
                                                     d_totals or None, d_err or None, stream or None))

    def batch(self, form, data, offsets):
        """Host numpy buffers in and out (hutk_normalize_batch): -> (bytes uint8, out_offsets int64[n + 1])."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0:
            raise TypeError("offsets must hold at least one entry")
        if int(offsets[n]) > len(data):
            raise TypeError("offsets point outside data")
        L = load()
        out, oo = C.c_void_p(), C.c_void_p()
        raise_for(L.hutk_normalize_batch(self._h, form, data.ctypes.data if len(data) else None, offsets.ctypes.data, n,
                                         C.byref(out), C.byref(oo)))
        try:
            r_oo = np.frombuffer((C.c_int64 * (n + 1)).from_address(oo.value), dtype=np.int64).copy()
            total = int(r_oo[n])
            r_out = np.frombuffer((C.c_uint8 * max(total, 1)).from_address(out.value), dtype=np.uint8)[:total].copy()
        finally:
            L.hutk_host_free(out)
            L.hutk_host_free(oo)
        return r_out, r_oo


def norm_chunk_bytes():
    return load().hutk_debug_norm_chunk_bytes()


class Pretokenizer(_Owner):
    """Owns one hutk_pretokenizer (the split presets on the GPU, include/hutoken_amd.h): the class tables of
    hutoken_amd.pretokenize on one device, and the workspace of its calls."""
    _destroy = "hutk_pretokenizer_destroy"

    def __init__(self, blob, device=-1):
        h = C.c_void_p()
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
        raise_for(load().hutk_pretokenizer_create(C.byref(h), int(device), C.cast(buf, C.c_void_p), len(blob)))
        self._h = h

    def batch_device(self, preset, d_bytes, d_offsets, n_docs, n_bytes, d_word_bits, d_err=0, stream=0):
        """hutk_pretokenize_batch_device on raw device pointers (ints).  Asynchronous on `stream`, never synchronises."""
        raise_for(load().hutk_pretokenize_batch_device(self._h, preset, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                       d_word_bits or None, d_err or None, stream or None))

    def starts_device(self, d_word_bits, d_offsets, n_docs, n_bytes, d_before, d_starts=0, d_start_offsets=0, stream=0):
        """hutk_pretokenize_starts_device; d_starts == 0: the counting call."""
        raise_for(load().hutk_pretokenize_starts_device(self._h, d_word_bits or None, d_offsets or None, n_docs, n_bytes,
                                                        d_before or None, d_starts or None, d_start_offsets or None, stream or None))


def presplit_chunk_bytes():
    return load().hutk_debug_presplit_chunk_bytes()


WORDPIECE_INFO = ["format_version", "unidata", "blob_bytes", "chunk_bytes", "vocab_size", "table_slots", "flags", "unk_id"]


class WordPiece(_Owner):
    """Owns one hutk_wordpiece (WordPiece encoding on the GPU, include/hutoken_amd.h): the class tables of
    hutoken_amd.wordpiece, the vocabulary's table and, with WP_STRIP_ACCENTS, a normaliser, on one device."""
    _destroy = "hutk_wordpiece_destroy"

    def __init__(self, tables, norm_blob, lines, unk_token, prefix, max_input_chars_per_word, flags, device=-1):
        """lines: the vocabulary, a list of bytes; unk_token, prefix: bytes"""
        import numpy as np
        h = C.c_void_p()
        tb = (C.c_uint8 * max(len(tables), 1)).from_buffer_copy(bytes(tables) or b"\0")
        nb = (C.c_uint8 * max(len(norm_blob), 1)).from_buffer_copy(bytes(norm_blob) or b"\0") if norm_blob else None
        offs = np.zeros(len(lines) + 1, dtype=np.int64)
        if lines:
            np.cumsum(np.fromiter(map(len, lines), dtype=np.int64, count=len(lines)), out=offs[1:])
        data = np.frombuffer(b"".join(lines) or b"\0", dtype=np.uint8)
        raise_for(load().hutk_wordpiece_create(C.byref(h), int(device), C.cast(tb, C.c_void_p), len(tables),
                                               C.cast(nb, C.c_void_p) if nb is not None else None, len(norm_blob) if norm_blob else 0,
                                               data.ctypes.data, offs.ctypes.data, len(lines), bytes(unk_token), bytes(prefix),
                                               int(max_input_chars_per_word), int(flags)))
        self._h = h

    def info(self):
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_wordpiece_info(self._h, out.ctypes.data))
        return dict(zip(WORDPIECE_INFO, out.tolist()))

    def ids_capacity(self, n_bytes, n_docs):
        return load().hutk_wordpiece_ids_capacity(self._h, n_bytes, n_docs)

    def bucket(self, piece, continuation):
        """hutk_debug_wordpiece_bucket: the slot the probe of `piece` (bytes) starts at"""
        buf = (C.c_uint8 * max(len(piece), 1)).from_buffer_copy(bytes(piece) or b"\0")
        return load().hutk_debug_wordpiece_bucket(self._h, C.cast(buf, C.c_void_p), len(piece), 1 if continuation else 0)

    def batch_device(self, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets, d_word_ids=0, d_err=0, stream=0):
        """hutk_wordpiece_encode_batch_device on raw device pointers (ints).  Asynchronous on `stream`, never synchronises."""
        raise_for(load().hutk_wordpiece_encode_batch_device(self._h, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                            d_ids or None, ids_cap, d_out_offsets or None, d_word_ids or None,
                                                            d_err or None, stream or None))

    def batch(self, data, offsets, word_ids=False):
        """Host numpy buffers in and out (hutk_wordpiece_encode_batch): -> (ids int32, out_offsets int64[n + 1]) and, with
        word_ids, the word ids (int32)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0:
            raise TypeError("offsets must hold at least one entry")
        if int(offsets[n]) > len(data):
            raise TypeError("offsets point outside data")
        L = load()
        ids, oo, wi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        raise_for(L.hutk_wordpiece_encode_batch(self._h, data.ctypes.data if len(data) else None, offsets.ctypes.data, n,
                                                C.byref(ids), C.byref(oo), C.byref(wi) if word_ids else None))
        try:
            r_oo = np.frombuffer((C.c_int64 * (n + 1)).from_address(oo.value), dtype=np.int64).copy()
            total = int(r_oo[n])
            r_ids = np.frombuffer((C.c_int32 * max(total, 1)).from_address(ids.value), dtype=np.int32)[:total].copy()
            r_wi = np.frombuffer((C.c_int32 * max(total, 1)).from_address(wi.value), dtype=np.int32)[:total].copy() if word_ids else None
        finally:
            L.hutk_host_free(ids)
            L.hutk_host_free(oo)
            if word_ids:
                L.hutk_host_free(wi)
        return (r_ids, r_oo, r_wi) if word_ids else (r_ids, r_oo)


def wordpiece_chunk_bytes():
    return load().hutk_debug_wordpiece_chunk_bytes()


UNIGRAM_INFO = ["chunk_bytes", "vocab_size", "table_slots", "flags", "unk_id", "max_piece_bytes", "piece_bytes_bound", "group_lanes"]
UG_PREPEND, UG_WHITESPACE_SPLIT, UG_COLLAPSE_SPACES = 1, 2, 4


class Unigram(_Owner):
    """Owns one hutk_unigram (Unigram encoding on the GPU, include/hutoken_amd.h): the vocabulary's table and scores on
    one device."""
    _destroy = "hutk_unigram_destroy"

    def __init__(self, pieces, scores, unk_id, flags, device=-1):
        """pieces: the vocabulary, a list of bytes; scores: as many floats"""
        import numpy as np
        h = C.c_void_p()
        offs = np.zeros(len(pieces) + 1, dtype=np.int64)
        if pieces:
            np.cumsum(np.fromiter(map(len, pieces), dtype=np.int64, count=len(pieces)), out=offs[1:])
        data = np.frombuffer(b"".join(pieces) or b"\0", dtype=np.uint8)
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        raise_for(load().hutk_unigram_create(C.byref(h), int(device), data.ctypes.data, offs.ctypes.data,
                                             sc.ctypes.data if len(sc) else None, len(pieces), int(unk_id), int(flags)))
        self._h = h

    def info(self):
        import numpy as np
        out = np.zeros(8, dtype=np.int64)
        raise_for(load().hutk_unigram_info(self._h, out.ctypes.data))
        return dict(zip(UNIGRAM_INFO, out.tolist()))

    def ids_capacity(self, n_bytes, n_docs):
        return load().hutk_unigram_ids_capacity(self._h, n_bytes, n_docs)

    def bucket(self, piece):
        """hutk_debug_unigram_bucket: the slot the probe of `piece` (folded bytes) starts at"""
        buf = (C.c_uint8 * max(len(piece), 1)).from_buffer_copy(bytes(piece) or b"\0")
        return load().hutk_debug_unigram_bucket(self._h, C.cast(buf, C.c_void_p), len(piece))

    def batch_device(self, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets, d_word_ids=0, d_err=0, stream=0):
        """hutk_unigram_encode_batch_device on raw device pointers (ints).  Asynchronous on `stream`, never synchronises."""
        raise_for(load().hutk_unigram_encode_batch_device(self._h, d_bytes or None, d_offsets or None, n_docs, n_bytes,
                                                          d_ids or None, ids_cap, d_out_offsets or None, d_word_ids or None,
                                                          d_err or None, stream or None))

    def batch(self, data, offsets, word_ids=False):
        """Host numpy buffers in and out (hutk_unigram_encode_batch): -> (ids int32, out_offsets int64[n + 1]) and, with
        word_ids, the word ids (int32)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0:
            raise TypeError("offsets must hold at least one entry")
        if int(offsets[n]) > len(data):
            raise TypeError("offsets point outside data")
        L = load()
        ids, oo, wi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        raise_for(L.hutk_unigram_encode_batch(self._h, data.ctypes.data if len(data) else None, offsets.ctypes.data, n,
                                              C.byref(ids), C.byref(oo), C.byref(wi) if word_ids else None))
        try:
            r_oo = np.frombuffer((C.c_int64 * (n + 1)).from_address(oo.value), dtype=np.int64).copy()
            total = int(r_oo[n])
            r_ids = np.frombuffer((C.c_int32 * max(total, 1)).from_address(ids.value), dtype=np.int32)[:total].copy()
            r_wi = np.frombuffer((C.c_int32 * max(total, 1)).from_address(wi.value), dtype=np.int32)[:total].copy() if word_ids else None
        finally:
            L.hutk_host_free(ids)
            L.hutk_host_free(oo)
            if word_ids:
                L.hutk_host_free(wi)
        return (r_ids, r_oo, r_wi) if word_ids else (r_ids, r_oo)


def unigram_chunk_bytes():
    return load().hutk_debug_unigram_chunk_bytes()
