"""hutoken_amd -- MI355X-native batch BPE encode path behind huToken's Python surface.

`import hutoken_amd as hutoken` is the drop-in for the encode direction of the
reference's `hutoken` module (reference hutoken.py:22-43, 122-139):

    hutoken.initialize(vocab_file, special_chars_file, prefix=None, is_byte_encoder=False)
    hutoken.encode(text)                      -> list[int]
    hutoken.batch_encode(texts, num_threads)  -> list[list[int]]

Signatures, return types, exception classes and the messages the reference's tests
pin are kept.  Token ids are bit-exact with the reference's string-keyed path.
The work is done by hand-written HIP kernels behind the C ABI of
include/hutoken_amd.h; there is no CPU fallback: without the native library or a
GPU every call raises.

Also here (not in the reference): `encode_packed` / `encode_packed_device`, the
zero-marshalling entry points for packed UTF-8 + offsets.

Collation (not in the reference either): `collate_padded` / `batch_encode_padded` turn the device arrays of
`encode_packed_device` into padded rows with attention mask and lengths, `SequencePacker` into packed rows of
`seq_len` tokens with position and segment ids -- one HIP pass each (csrc/hutk_collate.hip).  `collate_windows` /
`batch_encode_windows` cut documents longer than `max_length` into overlapping windows (`stride`), every window a padded
row, with `row_map` from rows back to documents.  `collate_pairs` / `batch_encode_pairs` put two texts into one row,
[bos] A sep B [eos] with token type ids and the longest_first / only_first / only_second truncation;
`collate_pair_windows` / `batch_encode_pair_windows` cut the named side into overlapping windows instead.

Training targets (not in the reference): `mask_tokens` corrupts collated rows for masked-LM training and gives the
labels, by tokens or by whole words, with random numbers that are a stated function of (seed, row, column) or (seed, row,
side, word); `lm_labels` gives the loss labels of causal-LM and prompt + answer rows; `batch_encode_mlm` is the list
form -- one HIP pass each over rows that exist already (csrc/hutk_collate.hip, csrc/hutk_philox.h).  `corrupt_spans`
is the span corruption of T5-style encoder-decoder training: every noise span of a row becomes one sentinel, the row
closes up, and the spans move behind their sentinels into a target row, with the lengths of both and, on request, the
decoder's input; `batch_encode_span_corruption` is the list form.  One wavefront per row scans and compacts it.

Chat (not in the reference): `ChatTemplate` holds what surrounds the turns of a conversation (role headers, end-of-turn
markers, bos/eos; presets `chatml()` and `llama3()`); `render_chat_device` turns the turns' contents, encoded as one
document each, into one sequence per conversation -- a ragged pair that every collation above takes unchanged -- with
loss labels on the assistant turns only, turn ids and source indices; `batch_encode_chat` is the list form
(csrc/hutk_collate.hip).

Fill-in-the-middle (not in the reference): `fim_device` cuts the documents of a ragged pair into prefix / middle /
suffix and re-orders them behind three sentinel ids, PSM or SPM, with random numbers that are a stated function of
(seed, document) -- a ragged pair again, with loss labels, parts and source indices; `fim_cut_text_device` and
`fim_pieces_device` are the character-level form, which cuts the packed text BEFORE it is encoded so that no token
straddles a cut; `batch_encode_fim` is the list form (csrc/hutk_fim.h, csrc/hutk_collate.hip).

Best-fit packing (not in the reference): `pack_best_fit` lays the documents of a ragged pair into rows of `seq_len`
tokens WITHOUT cutting any that fits a row -- only a longer one is cut, every `seq_len` tokens, and the pieces are packed
best-fit-decreasing (Ding et al. 2024) -- with position and segment ids, lengths and, on request, the source index of
every element and the place of every document; `gather_source` moves any per-token array (labels, turn ids, spans, word
ids) along such a source array, the chat render's and fill-in-the-middle's too; `batch_encode_best_fit` is the list form.
The plan is made on the GPU, never on the host (csrc/hutk_bestfit.hip).

Offset mapping (not in the reference): `token_spans_device` turns the same device arrays plus the packed text into the
[start, end) of every token in its document, in characters or bytes; `batch_encode_with_offsets` and
`encode_with_offsets` are the list forms (csrc/hutk_spans.hip).

Special tokens (not in the reference, which cuts "<|endoftext|>" into eight ids): `set_special_tokens` installs
{string: id}; `encode_special`, `batch_encode_special` and `encode_special_packed_device` match them on the GPU and give
each ONE id, the text between them encoded as ever (csrc/hutk_special.hip).  `encode` / `batch_encode` never look at them.
`decode_special` / `batch_decode_special` turn such ids back into text (`skip_special_tokens=True` leaves the markers out),
`decode_packed_device` is the device-tensor form of both decodes; `decode` / `batch_decode` never look at the set either.

Byte fallback (not in the reference, which gives -1 for a character the vocabulary does not hold): `set_byte_fallback`
installs the ids of the vocabulary's `<0x00>`..`<0xFF>` lines (or 256 ids of the caller's); `encode_fallback`,
`batch_encode_fallback` and `encode_fallback_packed_device` replace every -1 by the ids of the bytes of the item it
covers, `decode_fallback` / `batch_decode_fallback` / `decode_packed_device(byte_fallback=True)` turn such ids back into
the raw bytes (csrc/hutk_fallback.hip).  Every other function ignores the table.

WordPiece (not in the reference, whose only encoder is BPE): `WordPiece` holds a BERT-family vocabulary (a vocab.txt
with "##" pieces) and encodes on the GPU as `tokenizers` does with BertNormalizer, BertPreTokenizer and
models.WordPiece: `encode_packed_device` gives the same ragged (ids, offsets) pair as the function of that name, and
word ids on request, so every collate_*, SequencePacker.add and mask_tokens takes it unchanged; `batch_encode` and
`encode` are the list forms, `from_file` and `from_tokenizer` the other constructors (csrc/hutk_wordpiece.hip, DESIGN.md
section 8m).  It needs no initialised context.

Unigram (not in the reference either): `Unigram` holds a SentencePiece-style Unigram vocabulary -- (piece, score) pairs
and an unk id, as T5, mT5, ALBERT, XLNet, XLM-R, mBART and Pegasus use -- and encodes on the GPU as `tokenizers` does with
models.Unigram behind a Metaspace pre-tokenizer: the Metaspace word split (or T5's whitespace split in front of it), then
the best path over every word's piece lattice in f64.  The methods and constructors are WordPiece's
(`encode_packed_device` with word ids on request, `batch_encode`, `encode`, `from_file` for a tokenizer.json,
`from_tokenizer`); csrc/hutk_unigram.hip, DESIGN.md section 8n.  It needs no initialised context.

Training (reference hutoken.py:163-171, src/lib.c:76-126) runs on the GPU too:
`bpe_train` / `bbpe_train` are the reference's entry points, `Trainer` and `train`
the batch-fed trainer and a writer of GPT-2-shaped (mode="bytes") or
SentencePiece/Llama-shaped (mode="chars") vocab, special and merges files.
"""
import os
import sys
import traceback

from . import _capi
from . import pretokenize as _presplit_tables  # (the module; the package's name `pretokenize` is the function below)
from . import normalize as _norm_tables  # (the module; the name `normalize` of the package is the function below)
from . import wordpiece as _wp_tables

__all__ = ["Unigram", "WordPiece", "packed_cu_seqlens", "packed_lm_labels", "corrupt_spans", "batch_encode_span_corruption", "mask_tokens", "lm_labels", "batch_encode_mlm", "gather_rows", "answer_positions", "token_word_ids_device", "initialize", "encode", "batch_encode", "encode_packed", "encode_packed_device",
           "decode", "batch_decode", "context", "Trainer", "train", "bpe_train", "bbpe_train",
           "collate_padded", "batch_encode_padded", "SequencePacker", "collate_windows", "batch_encode_windows",
           "token_spans_device", "batch_encode_with_offsets", "encode_with_offsets",
           "set_special_tokens", "encode_special", "batch_encode_special", "encode_special_packed_device",
           "decode_special", "batch_decode_special", "decode_packed_device",
           "set_byte_fallback", "encode_fallback", "batch_encode_fallback", "encode_fallback_packed_device",
           "decode_fallback", "batch_decode_fallback", "normalize_packed_device", "normalize",
           "pretokenize_packed_device", "pretokenize", "set_pretokenizer",
           "collate_pairs", "collate_pair_windows", "batch_encode_pairs", "batch_encode_pair_windows",
           "ChatTemplate", "render_chat_device", "batch_encode_chat",
           "fim_device", "fim_cut_text_device", "fim_pieces_device", "batch_encode_fim",
           "pack_best_fit", "gather_source", "batch_encode_best_fit"]

_NOT_INIT = ("Vocabulary is not initialized for encoding. "
             "Call 'initialize_encode' function first.")
_BAD_INIT_ARGS = ("Invalid arguments. Expected a string "
                  "(vocab_file_path), a string (special_file_path), "
                  "a string or None (prefix) a bool an"
                  "optional integer (special_token_id), "
                  " an optional string (regex_pattern) and"
                  "a string or None (merges_file_path)")

# process-global context, like the reference's global_encode_context (lib.c:73-74)
_ctx = None


def context():
    """The current hutoken_amd._capi.Context (None before initialize())."""
    return _ctx


def _native_initialize(vocab_file_path, special_file_path, prefix=None, is_byte_encoder=False,
                       special_token_id=-1, pattern=None, merges_file_path=None, device=-1, devices=None,
                       pretokenizer=None):
    # mirrors the argument contract of _hutoken.initialize (lib.c:188-215, "ss|zpizz")
    # devices (not in the reference): several GPUs of this process behind batch_encode (hutk_ctx_add_device)
    global _ctx
    if devices is None and os.environ.get("HUTOKEN_DEVICES"):
        devices = [int(x) for x in os.environ["HUTOKEN_DEVICES"].split(",") if x.strip()]
    if devices:
        device = int(devices[0])
    if not isinstance(vocab_file_path, str) or not isinstance(special_file_path, str) \
            or not (prefix is None or isinstance(prefix, str)) \
            or not (pattern is None or isinstance(pattern, str)) \
            or not (merges_file_path is None or isinstance(merges_file_path, str)) \
            or not isinstance(special_token_id, int):
        raise TypeError(_BAD_INIT_ARGS)
    if pretokenizer is not None:
        _presplit_tables.preset_index(pretokenizer)  # (an unknown name raises before anything is built)
    sh = _capi.shim()
    if sh is not None:
        # the compiled module with the reference's method table owns the context; this wrapper only looks at it
        sh.initialize(vocab_file_path, special_file_path, prefix, bool(is_byte_encoder), special_token_id, pattern,
                      merges_file_path, device)
        old, _ctx = _ctx, _capi.Context.from_handle(sh.handle())
        if old is not None:
            old.close()
        for d in (devices or [])[1:]:
            _ctx.add_device(int(d))
        if pretokenizer is not None:
            set_pretokenizer(pretokenizer)
        return None
    # merges_file_path: the id-keyed merge path (lib.c:573-663, core.c:211-337) on the same kernels
    new = _capi.Context(vocab_file_path, special_file_path, prefix, bool(is_byte_encoder), device,
                        merges_path=merges_file_path, devices=devices)
    if pattern is not None:
        # the regex pre-token path (core.c:350-360): libc's regexec finds the words on the host, pretokenizer and
        # merge loop run on the GPU
        try:
            new.set_pattern(pattern)
        except Exception:
            new.close()
            raise
    if pretokenizer is not None:
        try:
            new.set_pretokenizer(_presplit_tables.preset_index(pretokenizer), _presplit_tables.table_blob())
        except Exception:
            new.close()
            raise
    old, _ctx = _ctx, new
    if old is not None:
        old.close()
    return None


def initialize(model_or_path, *args, **kwargs):
    """hutoken.initialize (reference hutoken.py:22-120): local vocabulary files, or a Hugging Face
    model id / directory that `transformers` can resolve offline (see hutoken_amd/hf.py).

    Merges file: the reference's local-file branch checks that args[6] exists and then
    drops it (hutoken.py:30-43 never hands it to _hutoken.initialize); only its Hugging
    Face branch passes `merges_file_path=`.  The positional form is kept as it is; the
    keyword `merges_file_path=` (the native function's own name for it, lib.c:188-205)
    selects the id-keyed merge path here.

    pretokenizer= "gpt2", "cl100k" (alias "llama3") or "qwen2" (both branches): the word split of that tokenizer family,
    computed on the GPU in front of every encode (set_pretokenizer); absent: the built-in split, as before."""
    if os.path.isfile(model_or_path):
        special_chars_file = args[0] if args else None
        merges_file = args[6] if len(args) > 6 else None
        if special_chars_file and not os.path.isfile(special_chars_file):
            raise ValueError(f"Special characters file '{special_chars_file}' does not exist.")
        if merges_file and not os.path.isfile(merges_file):
            raise ValueError(f"The provided merges file '{merges_file}' does not exist.")
        prefix = kwargs.get("prefix", None)
        is_byte_encoder = kwargs.get("is_byte_encoder", False)
        token_id = kwargs.get("token_id", -1)
        regex_pattern = kwargs.get("pattern", None)
        device = kwargs.get("device", int(os.environ.get("HUTOKEN_DEVICE", "-1")))
        merges_kw = kwargs.get("merges_file_path", None)
        if merges_kw and not os.path.isfile(merges_kw):
            raise ValueError(f"The provided merges file '{merges_kw}' does not exist.")
        return _native_initialize(model_or_path, special_chars_file, prefix, is_byte_encoder, token_id,
                                  regex_pattern, merges_kw, device=device, devices=kwargs.get("devices", None),
                                  pretokenizer=kwargs.get("pretokenizer", None))
    # Hugging Face branch (hutoken.py:44-120): convert the tokenizer to huToken's files, then the same native
    # initialisation, on the id-keyed merge path when the tokenizer has merge rules
    from . import hf
    ex = hf.export(model_or_path, **kwargs)
    try:
        kw = {k: v for k, v in kwargs.items() if k not in ("is_byte_encoder",)}
        kw.setdefault("device", int(os.environ.get("HUTOKEN_DEVICE", "-1")))
        if "token_id" in kw:
            kw["special_token_id"] = kw.pop("token_id")
        return _native_initialize(ex["vocab_file"], ex["special_chars_file"], ex["prefix"], ex["is_byte_encoder"],
                                  *args, merges_file_path=ex["merges_file_path"], **kw)
    except Exception as e:
        traceback.print_exc(file=sys.stderr)
        raise RuntimeError("An unexpected error occured during "
                           f"initialization: {e}") from e


def _pack(texts):
    import numpy as np
    try:
        chunks = [t.encode("utf-8") for t in texts]  # a lone surrogate raises UnicodeEncodeError (reference: crash)
    except AttributeError:
        raise TypeError("bad argument type for built-in operation")
    data = b"".join(chunks)
    if b"\0" in data:  # rare: strdup() semantics of lib.c:770-772, a text ends at its first NUL
        chunks = [b if (z := b.find(b"\0")) < 0 else b[:z] for b in chunks]
        data = b"".join(chunks)
    offs = np.zeros(len(texts) + 1, dtype=np.int64)
    if chunks:
        np.cumsum(np.fromiter(map(len, chunks), dtype=np.int64, count=len(chunks)), out=offs[1:])
    return np.frombuffer(data, dtype=np.uint8), offs


def _rows(ids, oo, n):
    """ids and the n + 1 offsets into them (numpy arrays or tensors) -> the n lists of ids."""
    bounds = oo.tolist()
    flat = ids[:bounds[-1]].tolist()
    return [flat[bounds[i]:bounds[i + 1]] for i in range(n)]


def _texts(raw, oo, n):
    """Decoded bytes (a numpy array) and the n + 1 offsets into them -> the n str."""
    raw = raw.tobytes()
    bounds = oo.tolist()
    return [_ids_to_text(raw[bounds[i]:bounds[i + 1]]) for i in range(n)]


def _native_encode(text):
    sh = _capi.shim()
    if sh is not None:
        return sh.encode(text)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if not isinstance(text, str):
        raise TypeError(f"argument 1 must be str, not {type(text).__name__}")
    data = text.encode("utf-8")
    if b"\0" in data:
        raise ValueError("embedded null character")
    ids, _rc = _ctx.encode_one(data)  # an over-long word is not reported (lib.c:692-697)
    return ids


def _native_batch_encode(texts, num_threads=1):
    sh = _capi.shim()
    if sh is not None:
        return sh.batch_encode(texts, num_threads)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    if not isinstance(num_threads, int):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    data, offs = _pack(texts)
    if num_threads <= 0:
        return [[] for _ in texts]  # no worker starts (lib.c:784-791)
    # an over-long word ends its document silently, as in the reference (core.c:503)
    ids, oo, _st, _rc = _ctx.encode_packed(data, offs)
    return _rows(ids, oo, len(texts))


def encode(text):
    try:
        return _native_encode(text)
    except Exception as e:
        traceback.print_exc(file=sys.stderr)
        raise RuntimeError(f"hutoken: Error encoding text: {e}")


def batch_encode(texts, num_threads=1):
    try:
        return _native_batch_encode(texts, num_threads)
    except Exception as e:
        traceback.print_exc(file=sys.stderr)
        raise RuntimeError(f"hutoken: Error encoding texts: {e}")


def encode_packed(data, offsets):
    """Packed UTF-8 (uint8 array) + int64 offsets[n+1] on the host ->
    (ids int32 array, out_offsets int64[n+1], status int32[n]).  Raises like
    batch_encode."""
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    ids, oo, st, _rc = _ctx.encode_packed(data, offsets)
    return ids, oo, st


def encode_packed_device(d_bytes, d_offsets, check=True):
    """Device-resident torch tensors in (uint8 bytes, int64 offsets[n+1]), device
    tensors out: (ids int32[capacity], out_offsets int64[n+1]).  The ids of
    document i are ids[out_offsets[i]:out_offsets[i+1]].  Asynchronous on the
    current torch stream unless check=True, which synchronises and raises on a
    device-side error."""
    return _encode_on_current_stream("plain", d_bytes, d_offsets, 0, check)


def _encode_on_current_stream(kind, d_bytes, d_offsets, flags, check):
    """_encode_device where the docstrings say it runs: on torch's current stream, the default one included (which the
    C ABI would read as "the context's own stream": check=True then read the error word, and the caller the ids, before
    the kernels had run)."""
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    return _on_torch_stream(d_bytes.device, lambda: _encode_device(kind, d_bytes, d_offsets, flags, check),
                            used=(d_bytes, d_offsets))


def _encode_device(kind, d_bytes, d_offsets, flags, check):
    """What encode_packed_device ("plain"), encode_special_packed_device ("special") and encode_fallback_packed_device
    ("fallback", with its flags) share: the output tensors, the call on the current torch stream, the check."""
    import torch
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    n_docs = d_offsets.numel() - 1
    n_bytes = d_bytes.numel()
    cap = (_ctx.special_ids_capacity if kind == "special" or flags else _ctx.ids_capacity)(n_bytes, n_docs)
    dev = d_bytes.device
    ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    text = (d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes)
    out = (ids.data_ptr(), cap, oo.data_ptr(), 0, err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if kind == "fallback":
        _ctx.encode_fallback_device(*text, flags, *out)
    else:
        (_ctx.encode_special_device if kind == "special" else _ctx.encode_device)(*text, *out)
    if check:
        code = int(err.item())
        if kind == "fallback" and code == _capi.E_UNSUPPORTED:
            raise ValueError("hutoken_amd: encode_fallback_packed_device: a document's text does not hold the decoded bytes "
                             "of its tokens where their spans lie; it keeps its plain ids (device-side error %d)" % code)
        if code not in (0, _capi.E_WORD_TOO_LARGE):
            raise RuntimeError(f"hutoken_amd: device-side error {code}")
    return ids, oo


_NOT_INIT_DECODE = ("Vocabulary is not initialized for decoding. "
                    "Call 'initialize_decode' function first.")


def _ids_to_text(raw):
    # PyUnicode_FromString (lib.c:938-939): the C string ends at its first 0x00, then strict UTF-8
    z = raw.find(b"\0")
    return (raw if z < 0 else raw[:z]).decode("utf-8")


def _flat_ids(tokens, batch):
    """The argument checks of decode / batch_decode -> (ids int32, id_offsets int64)."""
    import numpy as np
    if not isinstance(tokens, list):
        raise TypeError("Failed to parse arguments. Expected a single list of tokens." if batch else
                        "Argument must be a list of integers")
    if _ctx is None:
        raise RuntimeError(_NOT_INIT_DECODE)
    if not batch:
        ids = np.asarray([int(t) for t in tokens], dtype=np.int64).astype(np.int32)  # (int)PyLong_AsLong
        return ids, np.array([0, len(ids)], dtype=np.int64)
    if len(tokens) <= 0:
        raise ValueError("No tokens provided.")
    for item in tokens:
        if not isinstance(item, list):
            raise TypeError("Each item must be a list of integers.")
    offs = np.zeros(len(tokens) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, tokens), dtype=np.int64, count=len(tokens)), out=offs[1:])
    flat = np.fromiter((int(t) for item in tokens for t in item), dtype=np.int64, count=int(offs[-1])).astype(np.int32)
    return flat, offs


def _decode_lists(packed, tokens, batch, *flags):
    """tokens (a list of ints; batch: a list of such lists) through the context's host decode named `packed`
    -> str (batch: list of str)."""
    ids, offs = _flat_ids(tokens, batch)
    out, oo, _st = getattr(_ctx, packed)(ids, offs, *flags)
    return _texts(out, oo, len(tokens)) if batch else _ids_to_text(out.tobytes())


def _rewrapped(tokens, batch, fn, *args):
    """fn(*args) with the exceptions of hutoken.decode (reference hutoken.py:140-151: a ValueError stays one and names
    the tokens) or, batch, of hutoken.batch_decode (hutoken.py:153-160)."""
    try:
        return fn(*args)
    except Exception as e:
        traceback.print_exc(file=sys.stderr)
        if isinstance(e, ValueError) and not batch:
            raise ValueError(f"hutoken: Error decoding tokens {tokens}: {e}")
        raise RuntimeError(f"hutoken: Error decoding tokens: {e}")


def _native_decode(tokens):
    """_hutoken.decode (lib.c:876-951): list[int] -> str."""
    sh = _capi.shim()
    if sh is not None:
        return sh.decode(tokens)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT_DECODE)
    return _decode_lists("decode_packed", tokens, False)


def _native_batch_decode(tokens, num_threads=1):
    """_hutoken.batch_decode (lib.c:954-1126): list[list[int]] -> list[str]."""
    sh = _capi.shim()
    if sh is not None:
        return sh.batch_decode(tokens, num_threads)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT_DECODE)
    return _decode_lists("decode_packed", tokens, True)


def decode(tokens):
    """hutoken.decode (reference hutoken.py:140-151)."""
    return _rewrapped(tokens, False, _native_decode, tokens)


def batch_decode(tokens, num_threads=1):
    """hutoken.batch_decode (reference hutoken.py:153-160)."""
    return _rewrapped(tokens, True, _native_batch_decode, tokens, num_threads)


# ---- training -------------------------------------------------------------------------------------------------
def _default_device(device):
    return int(os.environ.get("HUTOKEN_DEVICE", "-1")) if device is None else int(device)


_TRAIN_MODES = {"bytes": _capi.TRAIN_BYTES, "chars": _capi.TRAIN_CHARS}


def _train_mode(mode):
    if not isinstance(mode, str) or mode not in _TRAIN_MODES:
        raise ValueError("mode must be 'bytes' or 'chars', not %r" % (mode,))
    return _TRAIN_MODES[mode]


class Trainer:
    """BPE training on the GPU (hutk_trainer_*, include/hutoken_amd.h).  Documents arrive over any number of add() /
    add_packed() calls; run() once returns the merges.  Semantics: tools/train_vocab.cpp in the same mode:
    "bytes" (the 256 byte values are the initial symbols) or "chars" (words holding a control byte are dropped,
    ' ' becomes U+2581 and the initial symbols are the UTF-8 characters seen, sorted as byte strings)."""

    def __init__(self, device=None, mode="bytes"):
        self._t = _capi.Trainer(_default_device(device), _train_mode(mode))

    def add(self, texts):
        """A list of str, one document each (cut at the first NUL, like batch_encode)."""
        if not isinstance(texts, list):
            raise TypeError("Invalid arguments. Expected a list of strings.")
        data, offs = _pack(texts)
        self._t.add_packed(data, offs)

    def add_packed(self, data, offsets):
        """Packed bytes (uint8 array or bytes) + int64 offsets[n+1].  A 0x00 byte in a document raises ValueError
        and nothing of the call is counted."""
        import numpy as np
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(bytes(data), dtype=np.uint8)
        self._t.add_packed(data, offsets)

    def alphabet(self):
        """The initial symbols in id order, a list of bytes: the 256 single bytes in bytes mode, the characters of
        the kept words in chars mode.  Ends the adding phase: a later add() raises."""
        return self._t.alphabet()

    def run(self, n_merges):
        """-> (pairs int32[m, 2], counts int64[m]); merge k creates symbol len(alphabet()) + k (256 + k in bytes
        mode)."""
        if not isinstance(n_merges, int) or n_merges < 0:
            raise ValueError("n_merges must be a non-negative int")
        return self._t.run(n_merges)

    def stats(self):
        return self._t.stats()

    def debug_counters(self):
        """Counters of the internal paths add() and run() took (for tests)."""
        return self._t.debug_counters()

    def close(self):
        self._t.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _text_batches(texts):
    if isinstance(texts, list) and all(isinstance(t, str) for t in texts):
        yield texts
        return
    for batch in texts:
        if not isinstance(batch, list) or not all(isinstance(t, str) for t in batch):
            raise TypeError("texts must be a list of str or an iterable of such lists")
        yield batch


def train(texts, vocab_size, out_dir, name, end_of_text="<|endoftext|>", device=None, mode="bytes"):
    """Train on `texts` (a list of str, or an iterable of such lists fed batch by batch) and write the files of
    tools/make_vocab.py under out_dir: <name>_vocab.txt, <name>_special.txt, <name>_merges.txt.

    mode="bytes": GPT-2 shape (VG).  n_merges = vocab_size - 256 - (1 if end_of_text else 0).  The files load with
    initialize(vocab, special, is_byte_encoder=True).
    mode="chars": SentencePiece/Llama shape (VL): <unk>, <s>, </s>, <0x00>..<0xFF>, the alphabet (A characters), then
    the merges; n_merges = vocab_size - 259 - A, and a vocab_size below 259 + A raises RuntimeError before the merge
    loop.  end_of_text is not used.  The files load with initialize(vocab, special, prefix="▁",
    is_byte_encoder=False).

    -> dict(vocab_file, special_file, merges_file, n_merges, stats), and alphabet_size in chars mode."""
    from . import vocab_files as vf
    if not isinstance(vocab_size, int) or isinstance(vocab_size, bool):
        raise TypeError("vocab_size must be an int")
    if not isinstance(out_dir, str) or not isinstance(name, str):
        raise TypeError("out_dir and name must be str")
    if end_of_text is not None and not isinstance(end_of_text, str):
        raise TypeError("end_of_text must be a str or None")
    chars = _train_mode(mode) == _capi.TRAIN_CHARS
    if chars:
        if vocab_size < vf.LLAMA_FIXED_TOKENS:
            raise RuntimeError("vocab_size must be at least %d (3 special and 256 byte-fallback tokens) in chars mode."
                               % vf.LLAMA_FIXED_TOKENS)
    else:
        n_merges = vocab_size - 256 - (1 if end_of_text else 0)
        if n_merges < 0:
            raise RuntimeError("vocab_size must be at least 256 to encode all bytes.")
    if not os.path.isdir(out_dir):
        raise FileNotFoundError(f"out_dir '{out_dir}' does not exist.")
    with Trainer(device, mode) as t:
        for batch in _text_batches(texts):
            t.add(batch)
        if chars:
            alphabet = t.alphabet()
            n_merges = vocab_size - vf.LLAMA_FIXED_TOKENS - len(alphabet)
            if n_merges < 0:
                raise RuntimeError("vocab_size %d is below %d + A = %d: the corpus has A = %d distinct characters."
                                   % (vocab_size, vf.LLAMA_FIXED_TOKENS, vf.LLAMA_FIXED_TOKENS + len(alphabet),
                                      len(alphabet)))
        pairs, _counts = t.run(n_merges)
        stats = t.stats()
    if chars:
        out = vf.write_llama_files(out_dir, name, alphabet, pairs.tolist())
        out["alphabet_size"] = len(alphabet)
    else:
        out = vf.write_gpt2_files(out_dir, name, pairs.tolist(), end_of_text)
    out["n_merges"] = int(len(pairs))
    out["stats"] = stats
    return out


def _check_train_args(args, kwargs):
    # PyArg_ParseTuple(args, "sis", ...) of lib.c:81-83, then the checks of lib.c:85-95
    if kwargs:
        raise TypeError("function takes no keyword arguments")
    if len(args) != 3:
        raise TypeError(f"function takes exactly 3 arguments ({len(args)} given)")
    data, vocab_size, name = args
    if not isinstance(data, str):
        raise TypeError(f"argument 1 must be str, not {type(data).__name__}")
    if isinstance(vocab_size, float) or not hasattr(vocab_size, "__index__"):
        raise TypeError(f"'{type(vocab_size).__name__}' object cannot be interpreted as an integer")
    if not isinstance(name, str):
        raise TypeError(f"argument 3 must be str, not {type(name).__name__}")
    if "\0" in data or "\0" in name:
        raise ValueError("embedded null character")
    vocab_size = int(vocab_size)
    if vocab_size < 256:
        raise RuntimeError("vocab_size must be at least 256 to encode all bytes.")
    if len(name.encode("utf-8")) < 4 or not name.encode("utf-8").endswith(b".txt"):
        raise RuntimeError("vocab_file_name file extension must be .txt.")
    return data, vocab_size, name


def _native_bpe_train(which, args, kwargs):
    data, vocab_size, name = _check_train_args(args, kwargs)
    sh = _capi.shim()
    if sh is not None:
        return getattr(sh, which)(data, vocab_size, name)
    from . import vocab_files as vf
    import numpy as np
    raw = data.encode("utf-8")
    with Trainer(None) as t:
        t.add_packed(np.frombuffer(raw, dtype=np.uint8), np.array([0, len(raw)], dtype=np.int64))
        pairs, _ = t.run(vocab_size - 255)
    home = os.environ.get("HOME")
    if home is None:
        sys.stderr.write("Unable to get HOME environment variable.")
        return None
    d = os.path.join(home, "config")
    if os.path.isdir(d):
        print(f"Directory already exists: {d}")
    else:
        os.mkdir(d, 0o700)
        print(f"Directory created: {d}")
    path = f"{d}/{name}"
    with open(path, "w", encoding="ascii", newline="") as f:
        f.write(vf.raw_vocab_text(pairs.tolist(), vocab_size))
    print(f"Vocab saved to: {path}")
    sys.stdout.flush()
    return None


def bpe_train(*args, **kwargs):
    """hutoken.bpe_train(data, vocab_size, vocab_file_name) (reference hutoken.py:163-166, lib.c:76-101): trains on
    `data` as one document and writes $HOME/config/<vocab_file_name>.  The file is a raw-byte vocabulary that
    initialize(path) accepts: bytes 0x01..0xFF are ids 0..254, merge k is id 255 + k, at most vocab_size lines."""
    return _native_bpe_train("bpe_train", args, kwargs)


def bbpe_train(*args, **kwargs):
    """hutoken.bbpe_train (reference hutoken.py:168-171, lib.c:103-126): the same byte-level model as bpe_train."""
    return _native_bpe_train("bbpe_train", args, kwargs)


# ---- collation ------------------------------------------------------------------------------------------------
# The checks below run before any device call (and before torch is needed for anything but the tensors themselves).
_INT32_MIN, _INT32_MAX = -2**31, 2**31 - 1


def _token_arg(name, v, optional=True):
    """bos_id / eos_id / pad_id -> int32 value; None -> the C ABI's "absent" (HUTK_NO_TOKEN)."""
    if v is None and optional:
        return _capi.NO_TOKEN
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError("%s must be an int%s, not %s" % (name, " or None" if optional else "", type(v).__name__))
    if not (_INT32_MIN < v <= _INT32_MAX):
        raise ValueError("%s must fit an int32 (and not be its lowest value)" % name)
    return v


def _length_arg(name, v, least):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError("%s must be an int, not %s" % (name, type(v).__name__))
    if v < least or v > _INT32_MAX:
        raise ValueError("%s must be at least %d (1, and the bos/eos tokens must fit) and below 2**31" % (name, least))
    return v


def _out_width(dtype):
    """torch.int32 / torch.int64 (or their names; None: int32) -> (4 | 8, name)."""
    name = "int32" if dtype is None else dtype if isinstance(dtype, str) else str(dtype).rpartition(".")[2]
    if name not in ("int32", "int64"):
        raise ValueError("dtype must be torch.int32 or torch.int64, not %r" % (dtype,))
    return (4 if name == "int32" else 8), name


def _device_tensors(named, sizes):
    """named: (name, tensor, dtype name) of every argument that must be a one-dimensional contiguous torch tensor of that
    dtype on the GPU.  What can be said without a GPU is said first: sizes() raises what the caller asks of the tensors'
    lengths once they are known to be tensors of one dimension."""
    for name, t, want in named:
        if not (hasattr(t, "data_ptr") and hasattr(t, "is_cuda") and hasattr(t, "dtype")):
            raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
        if str(t.dtype).rpartition(".")[2] != want:
            raise TypeError("%s must have dtype %s, not %s" % (name, want, t.dtype))
    for name, t, _want in named:
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be one-dimensional and contiguous" % name)
    sizes()
    for name, t, _want in named:
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU: the collation runs there and nowhere else" % name)


def _ragged_args(ids, offsets, n_ids):
    """The (ids, offsets) pair of encode_packed_device: device tensors, int32 and int64[n_docs + 1]."""
    def sizes():
        if offsets.numel() < 1:
            raise ValueError("offsets must hold at least one entry")
    _device_tensors((("ids", ids, "int32"), ("offsets", offsets, "int64")), sizes)
    if ids.device != offsets.device:
        raise ValueError("ids and offsets must be on the same device")
    if n_ids is not None:
        if isinstance(n_ids, bool) or not isinstance(n_ids, int):
            raise TypeError("n_ids must be an int or None")
        if n_ids < 0 or n_ids > ids.numel():
            raise ValueError("n_ids must be in 0 .. ids.numel()")


def _n_ids(ids, offsets, n_ids):
    if n_ids is None:
        n_ids = int(offsets[-1].item())  # the one synchronisation; pass n_ids= to avoid it
        if n_ids < 0 or n_ids > ids.numel():
            raise ValueError("offsets[-1] = %d does not fit ids (%d elements)" % (n_ids, ids.numel()))
    return n_ids


def _raise_device_error(err, what):
    code = int(err.item())
    if code:
        raise ValueError("hutoken_amd: %s: device-side error %d (offsets that do not describe ids)" % (what, code))


def _n_rows_arg(n_rows):
    if n_rows is not None:
        if isinstance(n_rows, bool) or not isinstance(n_rows, int):
            raise TypeError("n_rows must be an int or None")
        if n_rows < 0:
            raise ValueError("n_rows must not be negative")


def _row_tensors(dev, n_rows, max_length, dname, types=False, row_map=False):
    """The outputs of a row layout, in the order the collate_* functions return them:
    (input_ids, attention_mask[, token_type_ids], lengths[, row_map])."""
    import torch
    res = [torch.empty((n_rows, max_length), dtype=getattr(torch, dname), device=dev),
           torch.empty((n_rows, max_length), dtype=torch.uint8, device=dev)]
    if types:
        res.append(torch.empty((n_rows, max_length), dtype=torch.uint8, device=dev))
    res.append(torch.empty(n_rows, dtype=torch.int32, device=dev))
    if row_map:
        res.append(torch.empty((n_rows, 2), dtype=torch.int64, device=dev))
    return tuple(res)


_SIDES = ("right", "left")


def collate_padded(ids, offsets, max_length=None, *, bos_id=None, eos_id=None, pad_id=0, truncation="right",
                   padding_side="right", dtype=None, n_ids=None, check=False, return_plan=False):
    """Device tensors of encode_packed_device in, a padded batch out, on the current torch stream:
    -> (input_ids [n_docs, max_length] of `dtype` (torch.int32, the default, or torch.int64),
        attention_mask uint8 [n_docs, max_length], lengths int32 [n_docs]).
    Row i is [bos_id] + ids[offsets[i]:offsets[i+1]] + [eos_id] (those given); a longer one keeps bos/eos and the
    first (truncation="right") or last ("left") max_length - s of the document's ids; pad_id fills the rest on
    `padding_side`.  max_length=None pads to the longest sequence (one small synchronising read); a given one
    synchronises only to read offsets[-1], and not at all with n_ids=.  check=True synchronises and raises ValueError
    when the kernel found offsets that do not describe ids.  return_plan=True appends row_plan int64 [n_docs, 8], the
    rows' geometry for gather_rows and answer_positions (one more launch on the same stream, no synchronisation)."""
    bos, eos, pad = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
    s = (bos != _capi.NO_TOKEN) + (eos != _capi.NO_TOKEN)
    if max_length is not None:
        _length_arg("max_length", max_length, max(1, s))
    if truncation not in _SIDES:
        raise ValueError("truncation must be 'right' or 'left', not %r" % (truncation,))
    if padding_side not in _SIDES:
        raise ValueError("padding_side must be 'right' or 'left', not %r" % (padding_side,))
    width, dname = _out_width(dtype)
    _ragged_args(ids, offsets, n_ids)
    import torch
    dev = ids.device
    n_docs = offsets.numel() - 1
    n_ids = _n_ids(ids, offsets, n_ids)
    if max_length is None:
        longest = int((offsets[1:] - offsets[:-1]).max().item()) if n_docs else 0
        max_length = _length_arg("max_length", max(1, s, longest + s), 1)
    out, mask, lengths = _row_tensors(dev, n_docs, max_length, dname)
    err = torch.zeros(2 if return_plan else 1, dtype=torch.int32, device=dev)  # one word per call
    flags = (_capi.COLLATE_TRUNC_LEFT if truncation == "left" else 0) | \
            (_capi.COLLATE_PAD_LEFT if padding_side == "left" else 0)
    plan = torch.empty((n_docs, 8), dtype=torch.int64, device=dev) if return_plan else None
    with torch.cuda.device(dev):
        _capi.collate_padded_device(ids.data_ptr(), offsets.data_ptr(), n_docs, n_ids, max_length, bos, eos, pad, flags,
                                    width, out.data_ptr(), mask.data_ptr(), lengths.data_ptr(), err.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream)
        if return_plan:
            _capi.padded_plan_device(offsets.data_ptr(), n_docs, n_ids, max_length, bos, eos, flags, plan.data_ptr(),
                                     err[1:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if check:
        _raise_device_error(err.max(), "collate_padded")
    return (out, mask, lengths, plan) if return_plan else (out, mask, lengths)


def _stride_arg(stride, room):
    """stride -> int in 0 .. room - 1 (room: the document ids a row holds)."""
    if isinstance(stride, bool) or not isinstance(stride, int):
        raise TypeError("stride must be an int, not %s" % type(stride).__name__)
    if stride < 0 or stride >= room:
        raise ValueError("stride must be in 0 .. %d (below max_length less the bos/eos tokens), not %d" % (room - 1, stride))
    return stride


def collate_windows(ids, offsets, max_length, stride=0, *, bos_id=None, eos_id=None, pad_id=0, padding_side="right",
                    dtype=None, n_ids=None, n_rows=None, check=False, return_plan=False):
    """Device tensors of encode_packed_device in, every document as overlapping windows out, on the current torch stream:
    -> (input_ids [n_rows, max_length] of `dtype` (torch.int32, the default, or torch.int64),
        attention_mask uint8 [n_rows, max_length], lengths int32 [n_rows], row_map int64 [n_rows, 2]).
    With C = max_length - (bos/eos tokens given) and step = C - stride, a document of n <= C ids is one row (an empty one
    too); a longer one gives 1 + ceil((n - C) / step) rows, row k holding [bos_id] + its ids [k * step, k * step + C) +
    [eos_id]; consecutive rows share `stride` ids and the last one is the short one.  Rows are padded with pad_id on
    `padding_side`; lengths counts bos/eos.  row_map[r] = (document, k * step): element q of unpadded row r that is not
    bos or eos is ids[offsets[document] + k * step + q - (1 with a bos_id)], so its span is that row of
    token_spans_device's result.  One small synchronising read gives the number of rows (and one more offsets[-1]);
    n_rows= and n_ids= avoid them.  check=True synchronises and raises ValueError when the kernels found offsets that do
    not describe ids or an n_rows that is not the number of rows.  return_plan=True appends row_plan int64 [n_rows, 8]
    (see collate_padded)."""
    bos, eos, pad = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
    s = (bos != _capi.NO_TOKEN) + (eos != _capi.NO_TOKEN)
    _length_arg("max_length", max_length, s + 1)
    _stride_arg(stride, max_length - s)
    if padding_side not in _SIDES:
        raise ValueError("padding_side must be 'right' or 'left', not %r" % (padding_side,))
    width, dname = _out_width(dtype)
    _n_rows_arg(n_rows)
    _ragged_args(ids, offsets, n_ids)
    import torch
    dev = ids.device
    n_docs = offsets.numel() - 1
    n_ids = _n_ids(ids, offsets, n_ids)
    row_offsets = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(3 if return_plan else 2, dtype=torch.int32, device=dev)  # one word per call
    plan = None
    flags = _capi.COLLATE_PAD_LEFT if padding_side == "left" else 0
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.windows_rows_device(offsets.data_ptr(), n_docs, n_ids, max_length, stride, bos, eos,
                                  row_offsets.data_ptr(), err[0:].data_ptr(), stream)
        if n_rows is None:
            n_rows = int(row_offsets[-1].item())  # the one synchronisation; pass n_rows= to avoid it
            if n_rows < n_docs or n_rows > _capi.windows_rows_bound(n_docs, n_ids, max_length, stride, s):
                raise ValueError("hutoken_amd: collate_windows: offsets that do not describe ids (%d rows)" % n_rows)
        out, mask, lengths, row_map = _row_tensors(dev, n_rows, max_length, dname, row_map=True)
        _capi.collate_windows_device(ids.data_ptr(), offsets.data_ptr(), row_offsets.data_ptr(), n_docs, n_ids, n_rows,
                                     max_length, stride, bos, eos, pad, flags, width, out.data_ptr(),
                                     mask.data_ptr(), lengths.data_ptr(), row_map.data_ptr(), err[1:].data_ptr(), stream)
        if return_plan:
            plan = torch.empty((n_rows, 8), dtype=torch.int64, device=dev)
            _capi.windows_plan_device(offsets.data_ptr(), row_offsets.data_ptr(), n_docs, n_ids, n_rows, max_length, stride,
                                      bos, eos, flags, plan.data_ptr(), err[2:].data_ptr(), stream)
    if check:
        _raise_device_error(err.max(), "collate_windows")
    return (out, mask, lengths, row_map, plan) if return_plan else (out, mask, lengths, row_map)


_side_streams = {}


def _on_torch_stream(dev, fn, used=()):
    """fn() -- calls of the C ABI on torch's current stream of `dev` -> what fn returns (a tensor, a tuple of them, None).
    The C ABI reads a NULL stream -- torch's default one -- as "the context's own stream", which no torch stream waits
    for.  So with that one current, fn runs on a stream of its own which waits for the current one and which the current
    one then waits for; the tensors in `used` are recorded on that stream, those fn returns on the current one."""
    import torch
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        if cur.cuda_stream:
            return fn()
        side = _side_streams.get(dev.index)
        if side is None:
            side = _side_streams[dev.index] = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            res = fn()
        cur.wait_stream(side)
        for t in used:
            t.record_stream(side)
        for t in () if res is None else res if isinstance(res, tuple) else (res,):
            t.record_stream(cur)
        return res


def _encode_texts(kind, texts, flags=0, with_text=False, normalize=None):
    """list of str -> (ids, out_offsets) of _encode_device(kind, ..., flags) on the context's device; with_text: and the
    packed text they were made from, (ids, out_offsets, d_bytes, d_offs).  The caller has checked texts and the context.
    normalize: a normal form ("NFC" ..) the packed text is put into on the GPU between upload and encode
    (normalize_packed_device: ids, spans and with_text are then those of the normalised text); None: the text as it is."""
    import torch
    _normalize_arg(normalize)
    data, offs = _pack(texts)
    dev = torch.device("cuda", _capi.load().hutk_device_ordinal(_ctx.handle))
    d_bytes = torch.from_numpy(data.copy()).to(dev)  # (a copy: _pack's array is a read-only view of a bytes object)
    d_offs = torch.from_numpy(offs).to(dev)
    if normalize is not None:
        with torch.cuda.device(dev):
            d_bytes, d_offs = normalize_packed_device(d_bytes, d_offs, normalize)
    ids, oo = _on_torch_stream(dev, lambda: _encode_device(kind, d_bytes, d_offs, flags, True))
    return (ids, oo, d_bytes, d_offs) if with_text else (ids, oo)


def _texts_to_device(texts, with_text=False, normalize=None):
    """list of str -> (ids, out_offsets) of encode_packed_device on the context's device; with_text: and the packed
    text they were made from, (ids, out_offsets, d_bytes, d_offs).  normalize: see _encode_texts."""
    _normalize_arg(normalize)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    return _encode_texts("plain", texts, 0, with_text, normalize)


def _feature_args(return_offsets_mapping, offsets_unit, return_word_ids):
    """What the batch_encode_* row functions check of their feature arguments before anything is encoded."""
    for name, v in (("return_offsets_mapping", return_offsets_mapping), ("return_word_ids", return_word_ids)):
        if not isinstance(v, bool):
            raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))
    _span_unit(offsets_unit)
    if return_word_ids and _ctx is not None and _ctx.pretokenizer is None:
        raise ValueError(_NO_PRESET)


def _rows_with_features(collate, kwargs, text, return_offsets_mapping, offsets_unit, return_word_ids):
    """collate(return_plan=..) -> its result with the rows' offset mapping and word ids appended, in that order: the
    per-token arrays of the one encode call (text: its ids, offsets and packed text) laid out by the rows' plan."""
    if not (return_offsets_mapping or return_word_ids):
        return collate(**kwargs)
    ids, oo, d_bytes, d_offs = text
    want_plan = kwargs.pop("return_plan", False)
    res = collate(return_plan=True, **kwargs)
    plan = res[-1]
    res = res if want_plan else res[:-1]
    max_length = res[0].shape[1]
    n_ids = int(oo[-1].item())
    if return_offsets_mapping:
        spans = token_spans_device(d_bytes, d_offs, ids, oo, unit=offsets_unit, n_ids=n_ids)
        res += (gather_rows(plan, max_length, spans, fill=0),)
    if return_word_ids:
        words = token_word_ids_device(d_bytes, d_offs, ids, oo, n_ids=n_ids)
        res += (gather_rows(plan, max_length, words, fill=-1),)
    return res


def batch_encode_padded(texts, max_length=None, *, normalize=None, return_offsets_mapping=False, offsets_unit="char",
                        return_word_ids=False, **collate_kwargs):
    """A list of str -> collate_padded's (input_ids, attention_mask, lengths): encode_packed_device, then
    collate_padded with `collate_kwargs`, both on the initialised context's GPU.  normalize="NFC" (.. "NFKD"): the
    texts are normalised on the GPU first (normalize_packed_device); None: they are encoded as they are.
    return_offsets_mapping=True appends offset_mapping int32 [n_rows, L, 2], the span of every token in its text in
    `offsets_unit` ("char" or "byte") and (0, 0) on the other columns; return_word_ids=True then appends word_ids int32
    [n_rows, L], the word of its text each token starts in and -1 on the other columns (token_word_ids_device: the
    context needs a split preset).  Both are token_spans_device / token_word_ids_device through gather_rows."""
    _feature_args(return_offsets_mapping, offsets_unit, return_word_ids)
    text = _texts_to_device(texts, with_text=True, normalize=normalize)
    return _rows_with_features(lambda **kw: collate_padded(text[0], text[1], max_length, **kw), collate_kwargs,
                               text, return_offsets_mapping, offsets_unit, return_word_ids)


def batch_encode_windows(texts, max_length, stride=0, *, normalize=None, return_offsets_mapping=False,
                         offsets_unit="char", return_word_ids=False, **collate_kwargs):
    """A list of str -> collate_windows' (input_ids, attention_mask, lengths, row_map): encode_packed_device, then
    collate_windows with `collate_kwargs`, both on the initialised context's GPU.  normalize, return_offsets_mapping,
    offsets_unit, return_word_ids: as batch_encode_padded."""
    _feature_args(return_offsets_mapping, offsets_unit, return_word_ids)
    text = _texts_to_device(texts, with_text=True, normalize=normalize)
    return _rows_with_features(lambda **kw: collate_windows(text[0], text[1], max_length, stride, **kw), collate_kwargs,
                               text, return_offsets_mapping, offsets_unit, return_word_ids)


_PAIR_STRATEGIES = {"longest_first": _capi.PAIR_LONGEST_FIRST, "only_first": _capi.PAIR_ONLY_FIRST,
                    "only_second": _capi.PAIR_ONLY_SECOND}


def _sep_arg(sep_ids):
    """sep_ids -> tuple of at most 4 int32 values, none of them the C ABI's "absent"."""
    if not isinstance(sep_ids, (tuple, list)):
        raise TypeError("sep_ids must be a tuple or list of ints, not %s" % type(sep_ids).__name__)
    if len(sep_ids) > _capi.PAIR_MAX_SEP:
        raise ValueError("sep_ids must hold at most %d ids, not %d" % (_capi.PAIR_MAX_SEP, len(sep_ids)))
    return tuple(_token_arg("sep_ids[%d]" % i, v, False) for i, v in enumerate(sep_ids))


def _pair_args(ids_a, offsets_a, ids_b, offsets_b):
    """The two ragged pairs of collate_pairs: device tensors on one device, as many documents on both sides."""
    four = (("ids_a", ids_a, "int32"), ("offsets_a", offsets_a, "int64"), ("ids_b", ids_b, "int32"),
            ("offsets_b", offsets_b, "int64"))

    def sizes():
        if offsets_a.numel() < 1:
            raise ValueError("offsets_a must hold at least one entry")
        if offsets_a.numel() != offsets_b.numel():
            raise ValueError("offsets_a and offsets_b must describe as many documents (%d and %d)"
                             % (offsets_a.numel() - 1, offsets_b.numel() - 1))
    _device_tensors(four, sizes)
    for name, t, _want in four:
        if t.device != ids_a.device:
            raise ValueError("%s must be on the same device as ids_a" % name)


def _pair_template(bos_id, sep_ids, eos_id, pad_id, truncation, padding_side, dtype):
    bos, eos, pad = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
    sep = _sep_arg(sep_ids)
    s = (bos != _capi.NO_TOKEN) + len(sep) + (eos != _capi.NO_TOKEN)
    if not isinstance(truncation, str) or truncation not in _PAIR_STRATEGIES:
        raise ValueError("truncation must be 'longest_first', 'only_first' or 'only_second', not %r" % (truncation,))
    if padding_side not in _SIDES:
        raise ValueError("padding_side must be 'right' or 'left', not %r" % (padding_side,))
    width, dname = _out_width(dtype)
    return bos, sep, eos, pad, s, _PAIR_STRATEGIES[truncation], width, dname


def collate_pairs(ids_a, offsets_a, ids_b, offsets_b, max_length=None, *, truncation="longest_first", bos_id=None,
                  sep_ids=(), eos_id=None, pad_id=0, padding_side="right", dtype=None, check=False, return_plan=False):
    """Two ragged pairs of one device in, one row per pair of documents out, on the current torch stream:
    -> (input_ids [n, max_length] of `dtype` (torch.int32, the default, or torch.int64), attention_mask uint8
        [n, max_length], token_type_ids uint8 [n, max_length], lengths int32 [n]).
    Row i is [bos_id] + A' + sep_ids + B' + [eos_id] with A = ids_a[offsets_a[i]:offsets_a[i+1]], B likewise; offsets_x[0]
    may be any base, so one encode_packed_device call over texts_a + texts_b serves both sides: ids_a = ids_b = ids,
    offsets_a = oo[:n+1], offsets_b = oo[n:].  With R = max_length - s ids of room (s: bos, separators, eos) both sides
    are cut on the right to (ka, kb): nothing when they fit; "longest_first" takes from the longer side until both are
    equal and then from both (the longer one keeps the odd id, B on a tie); "only_first" / "only_second" cut the named
    side, and the other one only when it alone exceeds R.  token_type_ids is 0 on bos, A' and the separators, 1 on B' and
    eos, 0 on padding; lengths is ka + kb + s.  max_length=None pads to the longest pair with nothing cut (one small
    synchronising read); a given one never synchronises.  check=True synchronises and raises ValueError when the kernel
    found offsets outside 0 <= offsets[0] <= .. <= offsets[n] <= ids.numel().  return_plan=True appends row_plan int64
    [n, 8] (see collate_padded)."""
    bos, sep, eos, pad, s, strategy, width, dname = _pair_template(bos_id, sep_ids, eos_id, pad_id, truncation,
                                                                   padding_side, dtype)
    if max_length is not None:
        _length_arg("max_length", max_length, s + 1)
    _pair_args(ids_a, offsets_a, ids_b, offsets_b)
    import torch
    dev = ids_a.device
    n = offsets_a.numel() - 1
    if max_length is None:
        both = (offsets_a[1:] - offsets_a[:-1]).clamp_(min=0) + (offsets_b[1:] - offsets_b[:-1]).clamp_(min=0)
        max_length = _length_arg("max_length", s + max(1, int(both.max().item()) if n else 1), s + 1)
    out, mask, types, lengths = _row_tensors(dev, n, max_length, dname, types=True)
    err = torch.zeros(2 if return_plan else 1, dtype=torch.int32, device=dev)  # one word per call
    flags = _capi.COLLATE_PAD_LEFT if padding_side == "left" else 0

    def call():
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.collate_pairs_device(ids_a.data_ptr(), offsets_a.data_ptr(), ids_b.data_ptr(), offsets_b.data_ptr(), 0, n,
                                   ids_a.numel(), ids_b.numel(), n, max_length, 0, strategy, bos, sep, eos, pad, flags,
                                   width, out.data_ptr(), mask.data_ptr(), types.data_ptr(), lengths.data_ptr(), 0,
                                   err.data_ptr(), stream)
        if not return_plan:
            return out, mask, types, lengths
        plan = torch.empty((n, 8), dtype=torch.int64, device=dev)
        _capi.pair_plan_device(offsets_a.data_ptr(), offsets_b.data_ptr(), 0, n, ids_a.numel(), ids_b.numel(), n, max_length,
                               0, strategy, bos, sep, eos, flags, plan.data_ptr(), err[1:].data_ptr(), stream)
        return out, mask, types, lengths, plan
    res = _on_torch_stream(dev, call, used=(ids_a, offsets_a, ids_b, offsets_b, err))
    if check:
        _raise_device_error(err.max(), "collate_pairs")
    return res


def collate_pair_windows(ids_a, offsets_a, ids_b, offsets_b, max_length, stride=0, *, truncation="only_second",
                         bos_id=None, sep_ids=(), eos_id=None, pad_id=0, padding_side="right", dtype=None, n_rows=None,
                         check=False, return_plan=False):
    """collate_pairs with the side `truncation` names ("only_second", the default, or "only_first") cut into overlapping
    windows instead of truncated -- question + long context for extractive QA:
    -> (input_ids, attention_mask, token_type_ids [n_rows, max_length], lengths int32 [n_rows], row_map int64 [n_rows, 2]).
    The other side keeps its first ko = min(its ids, R); the cut side of n ids has C = R - ko ids of room per row: one row
    when n <= C or C == 0 (the cut side is then empty), otherwise step = max(1, C - stride) and 1 + ceil((n - C) / step)
    rows, row k holding its ids [k * step, k * step + C) with the whole kept side; the last window is the short one.
    The rows of pair 0 come first, then those of pair 1, ..; row_map[r] = (pair, k * step), so the spans of the cut side
    are rows of token_spans_device's result.  "longest_first" is refused: its overflow is a cross product of both sides'
    windows.  One small synchronising read gives the number of rows; n_rows= avoids it.  check=True synchronises and
    raises ValueError for offsets outside their condition or an n_rows that is not the number of rows.  return_plan=True
    appends row_plan int64 [n_rows, 8] (see collate_padded)."""
    bos, sep, eos, pad, s, strategy, width, dname = _pair_template(bos_id, sep_ids, eos_id, pad_id, truncation,
                                                                   padding_side, dtype)
    if strategy == _capi.PAIR_LONGEST_FIRST:
        raise ValueError("truncation must be 'only_first' or 'only_second' here: the windows of 'longest_first' are a cross "
                         "product of both sides' windows, which this does not produce")
    _length_arg("max_length", max_length, s + 1)
    _stride_arg(stride, max_length - s)
    _n_rows_arg(n_rows)
    _pair_args(ids_a, offsets_a, ids_b, offsets_b)
    import torch
    dev = ids_a.device
    n = offsets_a.numel() - 1
    cap_a, cap_b = ids_a.numel(), ids_b.numel()
    bound = _capi.pair_rows_bound(n, cap_b if strategy == _capi.PAIR_ONLY_SECOND else cap_a, max_length, stride, s)
    if n_rows is not None and not n <= n_rows <= bound:
        raise ValueError("n_rows must be in %d .. %d (the pairs .. the pairs and the ids of the cut side), not %d"
                         % (n, bound, n_rows))
    row_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(3 if return_plan else 2, dtype=torch.int32, device=dev)  # one word per call
    flags = _capi.COLLATE_PAD_LEFT if padding_side == "left" else 0

    def call():
        nonlocal n_rows
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.pair_rows_device(offsets_a.data_ptr(), offsets_b.data_ptr(), n, cap_a, cap_b, max_length, stride, strategy,
                               bos, sep, eos, row_offsets.data_ptr(), err[0:].data_ptr(), stream)
        if n_rows is None:
            n_rows = int(row_offsets[-1].item())  # the one synchronisation; pass n_rows= to avoid it
            if not n <= n_rows <= bound:
                raise ValueError("hutoken_amd: collate_pair_windows: offsets that do not describe ids (%d rows)" % n_rows)
        out, mask, types, lengths, row_map = _row_tensors(dev, n_rows, max_length, dname, types=True, row_map=True)
        _capi.collate_pairs_device(ids_a.data_ptr(), offsets_a.data_ptr(), ids_b.data_ptr(), offsets_b.data_ptr(),
                                   row_offsets.data_ptr(), n, cap_a, cap_b, n_rows, max_length, stride, strategy, bos, sep,
                                   eos, pad, flags, width, out.data_ptr(), mask.data_ptr(), types.data_ptr(),
                                   lengths.data_ptr(), row_map.data_ptr(), err[1:].data_ptr(), stream)
        if not return_plan:
            return out, mask, types, lengths, row_map
        plan = torch.empty((n_rows, 8), dtype=torch.int64, device=dev)
        _capi.pair_plan_device(offsets_a.data_ptr(), offsets_b.data_ptr(), row_offsets.data_ptr(), n, cap_a, cap_b, n_rows,
                               max_length, stride, strategy, bos, sep, eos, flags, plan.data_ptr(), err[2:].data_ptr(), stream)
        return out, mask, types, lengths, row_map, plan
    res = _on_torch_stream(dev, call, used=(ids_a, offsets_a, ids_b, offsets_b, row_offsets, err))
    if check:
        _raise_device_error(err.max(), "collate_pair_windows")
    return res


def _pair_texts_to_device(texts_a, texts_b, normalize):
    """Two lists of str -> (ids, offsets_a, offsets_b, text): one encode of texts_a + texts_b, both sides views of its
    offsets; text: (ids, out_offsets, d_bytes, d_offsets) of that one call."""
    _normalize_arg(normalize)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if not isinstance(texts_a, list) or not isinstance(texts_b, list):
        raise TypeError("Invalid arguments. Expected two lists of strings.")
    if len(texts_a) != len(texts_b):
        raise ValueError("texts_a and texts_b must hold as many texts (%d and %d)" % (len(texts_a), len(texts_b)))
    n = len(texts_a)
    text = _encode_texts("plain", texts_a + texts_b, 0, True, normalize)
    return text[0], text[1][:n + 1], text[1][n:], text


def batch_encode_pairs(texts_a, texts_b, max_length=None, *, normalize=None, return_offsets_mapping=False,
                       offsets_unit="char", return_word_ids=False, **collate_kwargs):
    """Two lists of str -> collate_pairs' (input_ids, attention_mask, token_type_ids, lengths): one
    encode_packed_device call over texts_a + texts_b, then collate_pairs with `collate_kwargs` on views of its result,
    on the initialised context's GPU.  normalize, return_offsets_mapping, offsets_unit, return_word_ids: as
    batch_encode_padded; the spans and word ids of either side count from the start of that side's own text."""
    _feature_args(return_offsets_mapping, offsets_unit, return_word_ids)
    ids, oa, ob, text = _pair_texts_to_device(texts_a, texts_b, normalize)
    return _rows_with_features(lambda **kw: collate_pairs(ids, oa, ids, ob, max_length, **kw), collate_kwargs,
                               text, return_offsets_mapping, offsets_unit, return_word_ids)


def batch_encode_pair_windows(texts_a, texts_b, max_length, stride=0, *, normalize=None, return_offsets_mapping=False,
                              offsets_unit="char", return_word_ids=False, **collate_kwargs):
    """Two lists of str -> collate_pair_windows' (input_ids, attention_mask, token_type_ids, lengths, row_map); see
    batch_encode_pairs."""
    _feature_args(return_offsets_mapping, offsets_unit, return_word_ids)
    ids, oa, ob, text = _pair_texts_to_device(texts_a, texts_b, normalize)
    return _rows_with_features(lambda **kw: collate_pair_windows(ids, oa, ids, ob, max_length, stride, **kw), collate_kwargs,
                               text, return_offsets_mapping, offsets_unit, return_word_ids)


_PACKER_ROWS = ("input_ids", "position_ids", "segment_ids")


def _channel_specs(channels):
    """SequencePacker(channels=...): {name: (dtype, fill[, per])} -> [(name, dtype name, width, per, fill)], in the
    mapping's order.  Checked without a device."""
    if channels is None:
        return []
    if not isinstance(channels, dict):
        raise TypeError("channels must be a dict of name -> (dtype, fill[, per]), not %s" % type(channels).__name__)
    if len(channels) > _capi.PACKER_MAX_CHANNELS:
        raise ValueError("a packer carries at most %d channels, not %d" % (_capi.PACKER_MAX_CHANNELS, len(channels)))
    specs = []
    for name, spec in channels.items():
        if not isinstance(name, str) or not name:
            raise TypeError("a channel's name must be a non-empty str, not %r" % (name,))
        if name in _PACKER_ROWS:
            raise ValueError("a channel cannot be named %r: that is one of the packer's own outputs" % name)
        if not isinstance(spec, (tuple, list)) or len(spec) not in (2, 3):
            raise TypeError("channel %r must be given as (dtype, fill) or (dtype, fill, per)" % name)
        try:
            width, dname = _out_width(spec[0])
        except ValueError:
            raise ValueError("channel %r: dtype must be torch.int32 or torch.int64, not %r" % (name, spec[0])) from None
        if spec[0] is None:
            raise ValueError("channel %r: dtype must be torch.int32 or torch.int64, not None" % name)
        fill, per = spec[1], spec[2] if len(spec) == 3 else 1
        if isinstance(fill, bool) or not isinstance(fill, int):
            raise TypeError("channel %r: fill must be an int, not %s" % (name, type(fill).__name__))
        bits = 31 if dname == "int32" else 63
        if not -2**bits <= fill < 2**bits:
            raise ValueError("channel %r: fill must fit %s" % (name, dname))
        if isinstance(per, bool) or per not in (1, 2):
            raise ValueError("channel %r: per (the elements of a record) must be 1 or 2, not %r" % (name, per))
        specs.append((name, dname, width, per, fill))
    return specs


class SequencePacker:
    """Packs documents into rows of `seq_len` tokens for pretraining (hutk_packer_*, include/hutoken_amd.h).

    The stream is the documents' sequences end to end, each [bos_id] + ids + [eos_id] with the ids given; add()
    returns every complete row not yet returned as a dict of device tensors
        input_ids [rows, seq_len] (dtype), position_ids int32 (0 at every document start and row start),
        segment_ids int32 (1, 2, 3 .. per row, for masking attention at document boundaries)
    and keeps the unfinished row on the device for the next call; flush() returns it padded with pad_id (position 0,
    segment 0) and empties the stream.  The rows do not depend on how the documents are split over add() calls.

    channels={"labels": ("int64", -100), "spans": ("int32", 0, 2)}: name -> (dtype, fill[, per]), at most four.  A
    channel is a per-token array along the ids' offsets (labels and turn ids of render_chat_device, token spans, word
    ids) that the packer moves with the ids, carry included: add(..., channels={name: tensor}) then returns one more
    [rows, seq_len] tensor per channel ([rows, seq_len, 2] with per == 2) holding the token's value, and `fill` where
    the packer put bos, eos or padding."""

    _channels = ()  # (name, dtype name, width, per, fill) of each channel

    def __init__(self, seq_len, *, eos_id=None, bos_id=None, pad_id=0, dtype=None, device=None, channels=None):
        bos, eos, pad = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
        self.seq_len = _length_arg("seq_len", seq_len, 1)
        self._width, self._dname = _out_width(dtype)
        self._channels = _channel_specs(channels)
        if device is not None and (isinstance(device, bool) or not isinstance(device, int)):
            device = getattr(device, "index", device)  # a torch.device
            if device is not None and not isinstance(device, int):
                raise TypeError("device must be an int, a torch.device or None")
        self._p = _capi.Packer(self.seq_len, bos, eos, pad, self._width, _default_device(device),
                               channels=[(width, per, fill) for _n, _d, width, per, fill in self._channels])
        self._device = None

    @property
    def pending(self):
        """Tokens held for the next row."""
        return self._p.pending

    def _rows(self, n, dev):
        import torch
        shape = (n, self.seq_len)
        out = {"input_ids": torch.empty(shape, dtype=getattr(torch, self._dname), device=dev),
               "position_ids": torch.empty(shape, dtype=torch.int32, device=dev),
               "segment_ids": torch.empty(shape, dtype=torch.int32, device=dev)}
        for name, dname, _width, per, _fill in self._channels:
            out[name] = torch.empty(shape + ((2,) if per == 2 else ()), dtype=getattr(torch, dname), device=dev)
        return out

    def _channel_args(self, n_ids, channels):
        """add(channels=...): exactly the declared names, each a contiguous tensor of the declared dtype, [m] or [m, 2]
        by the declared record, with m >= n_ids (when n_ids is given) -> the tensors in the declared order.  No device
        is needed for any of it."""
        given = {} if channels is None else channels
        if not isinstance(given, dict):
            raise TypeError("channels must be a dict of name -> tensor, not %s" % type(given).__name__)
        names = [c[0] for c in self._channels]
        missing, extra = [n for n in names if n not in given], [n for n in given if n not in names]
        if missing or extra:
            raise ValueError("add() needs exactly the packer's channels %r: missing %r, not declared %r" % (names, missing, extra))
        for name, dname, _width, per, _fill in self._channels:
            t = given[name]
            if not _is_tensor(t):
                raise TypeError("channel %r must be a torch tensor, not %s" % (name, type(t).__name__))
            if _dtype_name(t) != dname:
                raise TypeError("channel %r must have dtype %s, not %s" % (name, dname, t.dtype))
            if not ((t.dim() == 1 and per == 1) or (t.dim() == 2 and per == 2 and t.shape[1] == 2)) or not t.is_contiguous():
                raise ValueError("channel %r must be contiguous and of shape %s" % (name, "[m, 2]" if per == 2 else "[m]"))
            if isinstance(n_ids, int) and t.shape[0] < n_ids:
                raise ValueError("channel %r holds %d records, fewer than n_ids = %d" % (name, t.shape[0], n_ids))
        return [given[n] for n in names]

    def add(self, ids, offsets, n_ids=None, check=False, channels=None):
        """Device tensors of encode_packed_device -> the complete rows (possibly zero), on the current torch stream.
        channels: name -> tensor for every channel the packer was made with (see the class); only the first n_ids
        records of each are read."""
        vals = self._channel_args(n_ids, channels)
        _ragged_args(ids, offsets, n_ids)
        for (name, *_rest), t in zip(self._channels, vals):
            if not t.is_cuda or t.device != ids.device:
                raise ValueError("channel %r must be on the device of ids" % name)
        import torch
        dev = ids.device
        n_docs = offsets.numel() - 1
        n_ids = _n_ids(ids, offsets, n_ids)
        for (name, *_rest), t in zip(self._channels, vals):
            if t.shape[0] < n_ids:
                raise ValueError("channel %r holds %d records, fewer than n_ids = %d" % (name, t.shape[0], n_ids))
        n = self._p.rows(n_docs, n_ids)
        out = self._rows(n, dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._device = dev
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            if self._channels:
                got = self._p.add_channels(ids.data_ptr(), offsets.data_ptr(), n_docs, n_ids, [t.data_ptr() for t in vals],
                                           out["input_ids"].data_ptr(), out["position_ids"].data_ptr(),
                                           out["segment_ids"].data_ptr(), [out[c[0]].data_ptr() for c in self._channels],
                                           n, err.data_ptr(), stream)
            else:
                got = self._p.add(ids.data_ptr(), offsets.data_ptr(), n_docs, n_ids, out["input_ids"].data_ptr(),
                                  out["position_ids"].data_ptr(), out["segment_ids"].data_ptr(), n, err.data_ptr(), stream)
        assert got == n
        if check:
            _raise_device_error(err, "SequencePacker.add")
        return out

    def add_texts(self, texts, normalize=None):
        """A list of str: encoded with the initialised context (encode_packed_device), then add().  normalize: as
        batch_encode_padded.  A packer with channels refuses: texts carry none."""
        if self._channels:
            raise ValueError("add_texts: the packer has channels %r and texts carry none; encode, build the channels and "
                             "call add()" % [c[0] for c in self._channels])
        ids, oo = _texts_to_device(texts, normalize=normalize)
        return self.add(ids, oo)

    def flush(self):
        """The unfinished row, padded (zero rows when nothing is pending); the stream starts anew."""
        import torch
        n = 1 if self._p.pending else 0
        dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
        out = self._rows(n, dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            with torch.cuda.device(dev):
                if self._channels:
                    self._p.flush_channels(out["input_ids"].data_ptr(), out["position_ids"].data_ptr(),
                                           out["segment_ids"].data_ptr(), [out[c[0]].data_ptr() for c in self._channels], stream)
                else:
                    self._p.flush(out["input_ids"].data_ptr(), out["position_ids"].data_ptr(),
                                  out["segment_ids"].data_ptr(), stream)
        return out

    def close(self):
        self._p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- token spans (offset mapping) ------------------------------------------------------------------------------------
_UNITS = {"char": _capi.SPANS_CHARS, "byte": _capi.SPANS_BYTES}


def _span_unit(unit):
    if unit not in _UNITS:
        raise ValueError("unit must be 'char' or 'byte', not %r" % (unit,))
    return _UNITS[unit]


def token_spans_device(d_bytes, d_offsets, ids, out_offsets, unit="char", dtype=None, n_ids=None, check=True):
    """The packed text (device tensors: uint8 bytes, int64 offsets[n_docs + 1]) and what encode_packed_device made of it
    (ids int32, out_offsets int64[n_docs + 1]) -> a device tensor [n_ids, 2] of `dtype` (torch.int32, the default, or
    torch.int64): token k of document i covers text_i[start:end] with (start, end) = spans[out_offsets[i] + k], counted in
    characters (unit="char", what str slicing takes) or bytes (unit="byte") from the document's start.  An id of -1 covers
    the one character (byte, with is_byte_encoder) at its place; the tokens of a prefix encoded on its own get (0, 0).
    On the current torch stream; synchronises only to read out_offsets[-1] (not with n_ids=) and for check=True, which
    raises ValueError naming the first document whose text does not hold its tokens' bytes, or TypeError for offsets
    that do not describe the tensors."""
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    code = _span_unit(unit)
    width, dname = _out_width(dtype)
    _ragged_args(ids, out_offsets, n_ids)
    for name, t, want in (("d_bytes", d_bytes, "uint8"), ("d_offsets", d_offsets, "int64")):
        if not (hasattr(t, "data_ptr") and hasattr(t, "is_cuda") and hasattr(t, "dtype")):
            raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
        if str(t.dtype).rpartition(".")[2] != want:
            raise TypeError("%s must have dtype %s, not %s" % (name, want, t.dtype))
        if t.dim() != 1 or not t.is_contiguous() or t.device != ids.device:
            raise ValueError("%s must be one-dimensional, contiguous and on the device of ids" % name)
    if d_offsets.numel() != out_offsets.numel():
        raise ValueError("d_offsets and out_offsets must describe the same documents")
    import torch
    dev = ids.device
    if dev.index != _capi.load().hutk_device_ordinal(_ctx.handle):
        raise ValueError("the tensors must be on the context's device: spans are computed there")
    n_docs = d_offsets.numel() - 1
    n_ids = _n_ids(ids, out_offsets, n_ids)
    spans = torch.empty((n_ids, 2), dtype=getattr(torch, dname), device=dev)
    status = torch.empty(max(n_docs, 1), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _ctx.token_spans_device(d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, d_bytes.numel(), ids.data_ptr(),
                                out_offsets.data_ptr(), n_ids, code, width, spans.data_ptr(), status.data_ptr(),
                                err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _on_torch_stream(dev, call, used=(d_bytes, d_offsets, ids, out_offsets, spans, status, err))
    if check:
        rc = int(err.item())
        if rc == _capi.E_ARG:
            raise TypeError("hutoken_amd: token_spans_device: offsets that do not describe the tensors (or a document of "
                            "2**31 bytes or more with int32 spans)")
        if rc:
            bad = torch.nonzero(status[:n_docs]).flatten()
            which = int(bad[0].item()) if bad.numel() else -1
            raise ValueError("hutoken_amd: token_spans_device: document %d: the text does not hold the decoded bytes of its "
                             "tokens where their spans lie (status %d, device-side error %d)"
                             % (which, int(status[which].item()) if which >= 0 else 0, rc))
    return spans


def batch_encode_with_offsets(texts, unit="char"):
    """A list of str -> (ids, offsets): ids as batch_encode returns them, offsets[i][k] = (start, end) of token k in
    texts[i], so that texts[i][start:end] is the text the token covers (unit="char"; "byte": in the UTF-8 bytes)."""
    _span_unit(unit)
    ids, oo, d_bytes, d_offs = _texts_to_device(texts, with_text=True)
    bounds = oo.cpu()  # (one copy down serves the spans' n_ids and both lists)
    spans = token_spans_device(d_bytes, d_offs, ids, oo, unit=unit, n_ids=int(bounds[-1]))
    return (_rows(ids, bounds, len(texts)),
            [[(a, b) for a, b in row] for row in _rows(spans, bounds, len(texts))])


def encode_with_offsets(text, unit="char"):
    """One str -> (ids, [(start, end), ...]); see batch_encode_with_offsets."""
    if not isinstance(text, str):
        raise TypeError(f"argument 1 must be str, not {type(text).__name__}")
    ids, spans = batch_encode_with_offsets([text], unit)
    return ids[0], spans[0]


# ---- special tokens ----------------------------------------------------------------------------------------------
def _special_pairs(mapping):
    """{str: int} -> [(utf-8 bytes, id)]; TypeError / ValueError before anything reaches the library."""
    if mapping is None:
        return []
    if not isinstance(mapping, dict):
        raise TypeError("special tokens must be a dict {str: int} or None, not %s" % type(mapping).__name__)
    pairs = []
    for k, v in mapping.items():
        if not isinstance(k, str):
            raise TypeError("a special token must be a str, not %s" % type(k).__name__)
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("the id of special token %r must be an int, not %s" % (k, type(v).__name__))
        raw = k.encode("utf-8")  # (a lone surrogate: UnicodeEncodeError, a ValueError)
        if not raw:
            raise ValueError("a special token must not be empty")
        if len(raw) > 255:
            raise ValueError("special token %r is longer than 255 bytes" % (k,))
        if b"\0" in raw:
            raise ValueError("special token %r holds a NUL character" % (k,))
        if not 0 <= v < 2**31:
            raise ValueError("the id of special token %r must be in [0, 2**31)" % (k,))
        pairs.append((raw, v))
    if len(pairs) > 1024:
        raise ValueError("at most 1024 special tokens")
    return pairs


def set_special_tokens(mapping):
    """Install special tokens on the initialised context: {str: int}, the strings as UTF-8; None or {} removes them.
    At most 1024 strings of 1..255 bytes without NUL, ids in [0, 2**31) that need not be vocabulary lines.  A new
    initialize() starts without any.  Only the *_special functions look at them."""
    pairs = _special_pairs(mapping)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    _ctx.set_special_tokens(pairs)


def encode_special_packed_device(d_bytes, d_offsets, check=True):
    """encode_packed_device with the special tokens of set_special_tokens: every match (leftmost first, then longest,
    inside one document) becomes its one id, the text between the matches is encoded as documents of its own.  Same
    tensors in, the same pair out -- (ids int32[capacity], out_offsets int64[n+1]) -- so collate_padded,
    SequencePacker.add and the spans' callers take it unchanged (spans over special ids are not defined), and
    decode_packed_device(ids, out_offsets, special=True) gives the text back.  Synchronises the current torch stream once,
    after the scan for matches."""
    return _encode_on_current_stream("special", d_bytes, d_offsets, 0, check)


def _special_texts_to_device(texts, normalize=None):
    """_texts_to_device for the special-token encode."""
    _normalize_arg(normalize)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    return _encode_texts("special", texts, normalize=normalize)


def batch_encode_special(texts, normalize=None):
    """batch_encode with the special tokens of set_special_tokens -> list[list[int]].  normalize: as
    batch_encode_padded (the special strings are matched in the normalised text)."""
    ids, oo = _special_texts_to_device(texts, normalize)
    return _rows(ids, oo, len(texts))


def encode_special(text):
    """encode with the special tokens of set_special_tokens -> list[int]."""
    if not isinstance(text, str):
        raise TypeError(f"argument 1 must be str, not {type(text).__name__}")
    if "\0" in text:
        raise ValueError("embedded null character")
    return batch_encode_special([text])[0]


def _skip_flag(skip_special_tokens):
    if not isinstance(skip_special_tokens, (bool, int)):
        raise TypeError("skip_special_tokens must be a bool, not %s" % type(skip_special_tokens).__name__)
    return _capi.DECODE_SKIP_SPECIAL if skip_special_tokens else 0


def decode_special(tokens, skip_special_tokens=False):
    """decode with the special tokens of set_special_tokens: a special id becomes its string (or nothing, with
    skip_special_tokens=True), and a context with a prefix strips it behind every marker, so that
    decode_special(encode_special(text)) == text.  Argument checks and exceptions are those of decode."""
    flags = _skip_flag(skip_special_tokens)
    return _rewrapped(tokens, False, _decode_lists, "decode_special_packed", tokens, False, flags)


def batch_decode_special(tokens, skip_special_tokens=False):
    """batch_decode with the special tokens of set_special_tokens -> list[str]; see decode_special."""
    flags = _skip_flag(skip_special_tokens)
    return _rewrapped(tokens, True, _decode_lists, "decode_special_packed", tokens, True, flags)


def decode_packed_device(d_ids, d_id_offsets, special=False, skip_special_tokens=False, n_ids=None, check=True,
                         byte_fallback=False):
    """The counterpart of encode_packed_device: device tensors in (ids int32, id_offsets int64[n+1], as the encode
    functions return them), device tensors out: (bytes uint8[total], out_offsets int64[n+1]); the text of document i is
    bytes[out_offsets[i]:out_offsets[i+1]].  special=False is the plain decode, special=True the one with the special
    tokens of set_special_tokens (encode_special_packed_device's ids), skip_special_tokens=True leaves their strings out.
    On the current torch stream: a sizes call, ONE synchronising read of the total, then the text call; n_ids= saves the
    read of id_offsets[-1].  check=True synchronises once more and raises ValueError for an id out of range and
    RuntimeError for a token that cannot be decoded on its own.  byte_fallback=True: the decode with the table of
    set_byte_fallback (an id of the table is its one raw byte), alone or together with special=True."""
    if not isinstance(special, (bool, int)):
        raise TypeError("special must be a bool, not %s" % type(special).__name__)
    if not isinstance(byte_fallback, (bool, int)):
        raise TypeError("byte_fallback must be a bool, not %s" % type(byte_fallback).__name__)
    flags = _skip_flag(skip_special_tokens)
    if flags and not special:
        raise ValueError("skip_special_tokens=True needs special=True: the plain decode knows no special tokens")
    _ragged_args(d_ids, d_id_offsets, n_ids)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT_DECODE)
    import torch
    dev = d_ids.device
    if dev.index != _capi.load().hutk_device_ordinal(_ctx.handle):
        raise ValueError("the tensors must be on the context's device: the decode runs there")
    n_docs = d_id_offsets.numel() - 1
    n_ids = _n_ids(d_ids, d_id_offsets, n_ids)
    oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    p_ids = d_ids.data_ptr() if n_ids else 0

    def call(out, cap):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if byte_fallback:
            fb = (_capi.FB_SPECIAL if special else 0) | (_capi.FB_SKIP_SPECIAL if flags else 0)
            _ctx.decode_fallback_device(p_ids, d_id_offsets.data_ptr(), n_docs, n_ids, fb, out, cap, oo.data_ptr(), 0,
                                        err.data_ptr(), stream)
        elif special:
            _ctx.decode_special_device(p_ids, d_id_offsets.data_ptr(), n_docs, n_ids, flags, out, cap, oo.data_ptr(), 0,
                                       err.data_ptr(), stream)
        else:
            _ctx.decode_device(p_ids or None, d_id_offsets.data_ptr(), n_docs, n_ids, out or None, cap, oo.data_ptr(), None,
                               err.data_ptr(), stream)

    def both():
        call(0, 0)
        total = int(oo[-1].item())  # the one synchronisation the result's size needs
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if total:
            call(out.data_ptr(), total)
        return out[:total]
    out = _on_torch_stream(dev, both, used=(d_ids, d_id_offsets, oo, err))
    if check:
        code = int(err.item())
        if code == _capi.E_VALUE:
            raise ValueError("hutoken_amd: decode_packed_device: Element must be non-negative and less than vocab size.")
        if code:
            raise RuntimeError("hutoken_amd: decode_packed_device: device-side error %d%s" % (
                code, " (a token cannot be decoded on its own)" if code == _capi.E_UNSUPPORTED else ""))
    return out, oo


# ---- byte fallback ---------------------------------------------------------------------------------------------------
def _fallback_table(table):
    """The argument of set_byte_fallback -> "auto", None or a list of 256 ints; TypeError / ValueError before anything
    reaches the library."""
    if table is None or (isinstance(table, str) and table == "auto"):
        return table
    if isinstance(table, (str, bytes)) or not hasattr(table, "__len__") or not hasattr(table, "__iter__"):
        raise TypeError('a byte-fallback table must be "auto", None or a sequence of 256 ints, not %s' % type(table).__name__)
    ids = list(table)
    for b, v in enumerate(ids):
        if isinstance(v, bool) or not isinstance(v, int):
            try:
                import numpy as np
                if isinstance(v, np.integer):
                    ids[b] = int(v)
                    continue
            except ImportError:
                pass
            raise TypeError("the id of byte 0x%02X must be an int, not %s" % (b, type(v).__name__))
    if len(ids) != 256:
        raise ValueError("a byte-fallback table holds 256 ids, not %d" % len(ids))
    for b, v in enumerate(ids):
        if not 0 <= v < 2**31:
            raise ValueError("the id of byte 0x%02X must be in [0, 2**31)" % b)
    if len(set(ids)) != 256:
        raise ValueError("two bytes of the byte-fallback table have the same id")
    return ids


def set_byte_fallback(table="auto"):
    """Install the byte-fallback table on the initialised context.  "auto": the ids of the vocabulary's 256 lines
    "<0x00>".."<0xFF>" (ValueError naming the first missing byte unless all are there); or a sequence of 256 distinct
    ints in [0, 2**31), the id of every byte value, which need not be vocabulary lines; None removes the table.  A new
    initialize() starts without one.  Only the *_fallback functions (and decode_packed_device(byte_fallback=True)) look
    at it: an item the vocabulary does not hold -- a -1 of encode -- becomes the ids of its bytes, and such an id decodes
    to its one raw byte."""
    ids = _fallback_table(table)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if isinstance(ids, str):
        found, n = _ctx.find_byte_tokens()
        if n != 256:
            b = int((found < 0).nonzero()[0][0])
            raise ValueError("the vocabulary has no line <0x%02X>: %d of the 256 byte-fallback lines were found" % (b, n))
        ids = found.tolist()
    _ctx.set_byte_fallback(ids)


def _special_arg(special):
    if not isinstance(special, (bool, int)):
        raise TypeError("special must be a bool, not %s" % type(special).__name__)
    return _capi.FB_SPECIAL if special else 0


def encode_fallback_packed_device(d_bytes, d_offsets, special=False, check=True):
    """encode_packed_device with the table of set_byte_fallback: every -1 of the plain encode is replaced, in place, by
    the ids of the bytes of the one item it covers.  Same tensors in, the same pair out: (ids int32[capacity], out_offsets
    int64[n+1]).  special=True also cuts at the special tokens of set_special_tokens, as encode_special_packed_device does
    (and then synchronises the current torch stream once); without it the call is asynchronous unless check=True, which
    synchronises and raises on a device-side error."""
    return _encode_on_current_stream("fallback", d_bytes, d_offsets, _special_arg(special), check)


def _fallback_texts_to_device(texts, special, normalize=None):
    """_texts_to_device for the fallback encode."""
    _normalize_arg(normalize)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    flags = _special_arg(special)
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    return _encode_texts("fallback", texts, flags, normalize=normalize)


def batch_encode_fallback(texts, special=False, normalize=None):
    """batch_encode with the table of set_byte_fallback -> list[list[int]]; special=True: and the special tokens.
    normalize: as batch_encode_padded."""
    ids, oo = _fallback_texts_to_device(texts, special, normalize)
    return _rows(ids, oo, len(texts))


def encode_fallback(text, special=False):
    """encode with the table of set_byte_fallback -> list[int]; special=True: and the special tokens."""
    if not isinstance(text, str):
        raise TypeError(f"argument 1 must be str, not {type(text).__name__}")
    if "\0" in text:
        raise ValueError("embedded null character")
    return batch_encode_fallback([text], special)[0]


def _fallback_decode_flags(special, skip_special_tokens):
    flags = _special_arg(special) | (_capi.FB_SKIP_SPECIAL if _skip_flag(skip_special_tokens) else 0)
    if flags & _capi.FB_SKIP_SPECIAL and not special:
        raise ValueError("skip_special_tokens=True needs special=True: without it the decode knows no special tokens")
    return flags


def decode_fallback(tokens, special=False, skip_special_tokens=False):
    """decode (special=True: decode_special) with the table of set_byte_fallback: an id of the table becomes its one raw
    byte, so that decode_fallback(encode_fallback(text)) == text.  Argument checks and exceptions are those of decode."""
    flags = _fallback_decode_flags(special, skip_special_tokens)
    return _rewrapped(tokens, False, _decode_lists, "decode_fallback_packed", tokens, False, flags)


def batch_decode_fallback(tokens, special=False, skip_special_tokens=False):
    """batch_decode with the table of set_byte_fallback -> list[str]; see decode_fallback."""
    flags = _fallback_decode_flags(special, skip_special_tokens)
    return _rewrapped(tokens, True, _decode_lists, "decode_fallback_packed", tokens, True, flags)


# ---- Unicode normalisation (hutk_normalize.hip) ----
_normalizers = {}


def _normalize_arg(form):
    """normalize= of the list-form entry points: None or one of the four forms (TypeError / ValueError otherwise)."""
    if form is not None:
        _norm_tables.form_index(form)
    return form


def _normalizer(dev):
    """The normaliser of a torch device: its tables are built once per process and uploaded once per device."""
    nz = _normalizers.get(dev.index)
    if nz is None:
        nz = _normalizers[dev.index] = _capi.Normalizer(_norm_tables.table_blob(), dev.index)
    return nz


def _packed_text_args(d_bytes, d_offsets):
    """The (bytes, offsets) pair of encode_packed_device: device tensors, uint8 and int64[n_docs + 1]."""
    for name, t, want in (("d_bytes", d_bytes, "uint8"), ("d_offsets", d_offsets, "int64")):
        if not (hasattr(t, "data_ptr") and hasattr(t, "is_cuda") and hasattr(t, "dtype")):
            raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
        if str(t.dtype).rpartition(".")[2] != want:
            raise TypeError("%s must have dtype %s, not %s" % (name, want, t.dtype))
    for name, t in (("d_bytes", d_bytes), ("d_offsets", d_offsets)):
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be one-dimensional and contiguous" % name)
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU: the normalisation runs there and nowhere else" % name)
    if d_offsets.numel() < 1:
        raise ValueError("d_offsets must hold at least one entry")
    if d_bytes.device != d_offsets.device:
        raise ValueError("d_bytes and d_offsets must be on the same device")


def normalize_packed_device(d_bytes, d_offsets, form="NFC", *, n_out=None, copy=False, return_changed=False, check=False):
    """Unicode normalisation of a packed batch on the GPU, in front of the encoders: device tensors in (uint8 bytes,
    int64 offsets[n+1], as encode_packed_device takes them), the same pair out -- (bytes uint8[n_out], offsets
    int64[n+1]), and `changed` uint8[n] (document i differs from its input) with return_changed=True.  Document by
    document the result is d.decode("utf-8", "surrogateescape") -> unicodedata.normalize(form, .) ->
    .encode("utf-8", "surrogateescape"): exact at any length, ill-formed bytes are copied and never reached across, a
    0x00 byte is a character like any other, documents are independent.  form: "NFC", "NFD", "NFKC" or "NFKD".

    Runs on the current torch stream: a sizes call, one synchronising read of the two totals (and the error word), a
    write call.  When no document changed and copy is False the write call is skipped and the INPUT tensors are
    returned.  n_out= (the output's size, known from an earlier call) avoids the synchronisation: both calls are
    enqueued and the text is always written; check=True then synchronises and raises on a device-side error, a wrong
    n_out included.  Offsets that do not describe d_bytes raise ValueError (with n_out=: only under check=True).

    Needs no initialised context and touches no vocabulary.  Token spans and offsets computed from the result are
    over the normalised text; nothing maps them back to the original bytes."""
    fi = _norm_tables.form_index(form)
    _packed_text_args(d_bytes, d_offsets)
    if n_out is not None and (isinstance(n_out, bool) or not isinstance(n_out, int)):
        raise TypeError("n_out must be an int or None")
    if n_out is not None and n_out < 0:
        raise ValueError("n_out must not be negative")
    import torch
    dev = d_bytes.device
    nz = _normalizer(dev)
    n_docs, n_bytes = d_offsets.numel() - 1, d_bytes.numel()
    with torch.cuda.device(dev):
        oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        changed = torch.empty(max(n_docs, 1), dtype=torch.uint8, device=dev)
        small = torch.zeros(4, dtype=torch.int64, device=dev)  # the two totals; the error words of the two calls
        totals, err = small.data_ptr(), small.data_ptr() + 16
        stream = torch.cuda.current_stream(dev).cuda_stream
        text = (fi, d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes)
        nz.batch_device(*text, 0, 0, oo.data_ptr(), changed.data_ptr(), totals, err, stream)
        if n_out is None:
            total, n_changed, code, _ = small.tolist()  # the one synchronisation
            _raise_normalize_error(code & 0xFFFFFFFF, n_out, total)
            if n_changed == 0 and not copy:
                return (d_bytes, d_offsets, changed[:n_docs]) if return_changed else (d_bytes, d_offsets)
            cap = total
        else:
            cap = n_out
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        nz.batch_device(*text, out.data_ptr(), cap, 0, 0, 0, err + 8, stream)
        if check:
            total, _n, code, code2 = small.tolist()
            _raise_normalize_error((code & 0xFFFFFFFF) or (code2 & 0xFFFFFFFF), n_out, total)
    out = out[:cap]
    return (out, oo, changed[:n_docs]) if return_changed else (out, oo)


def _raise_normalize_error(code, n_out, total):
    if code == _capi.E_CAPACITY:
        raise ValueError("hutoken_amd: normalize_packed_device: n_out = %d is below the %d bytes of the result" % (n_out, total))
    if code:
        raise ValueError("hutoken_amd: normalize_packed_device: device-side error %d (offsets that do not describe d_bytes)" % code)
    if n_out is not None and n_out != total:
        raise ValueError("hutoken_amd: normalize_packed_device: n_out = %d, the result has %d bytes" % (n_out, total))


def normalize(texts, form="NFC"):
    """A list of str -> the list of their normal forms ("NFC", "NFD", "NFKC", "NFKD"), computed on the current GPU
    (normalize_packed_device; no context is needed).  Equals [unicodedata.normalize(form, t) for t in texts]; lone
    surrogates U+DC80..U+DCFF pass through as the bytes they escape."""
    import numpy as np
    import torch
    _norm_tables.form_index(form)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    try:
        chunks = [t.encode("utf-8", "surrogateescape") for t in texts]
    except AttributeError:
        raise TypeError("Invalid arguments. Expected a list of strings.")
    offs = np.zeros(len(chunks) + 1, dtype=np.int64)
    if chunks:
        np.cumsum(np.fromiter(map(len, chunks), dtype=np.int64, count=len(chunks)), out=offs[1:])
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bytes = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()).to(dev)
    out, oo = normalize_packed_device(d_bytes, torch.from_numpy(offs).to(dev), form)
    raw, bounds = out.cpu().numpy().tobytes(), oo.tolist()
    return [raw[bounds[i]:bounds[i + 1]].decode("utf-8", "surrogateescape") for i in range(len(chunks))]


# ---- WordPiece (hutk_wordpiece.hip) ----
class WordPiece:
    """A WordPiece vocabulary and BERT's normaliser and word split, encoding on the GPU what the `tokenizers` package
    encodes with models.WordPiece behind normalizers.BertNormalizer and pre_tokenizers.BertPreTokenizer.

    vocab: the tokens in id order (a list of str; of two equal ones the later id wins).  unk_token must be one of them.
    strip_accents=None means "as lowercase".  device: a torch device, an index, or None for the current one; the
    tables are uploaded at the first call that needs the GPU, once.  Needs no initialised context.

    Left out: token spans over the original text, decoding, and matching "[MASK]"-style special strings inside text
    (they are split like any other text: "[", "mask", "]")."""

    def __init__(self, vocab, unk_token="[UNK]", continuing_subword_prefix="##", max_input_chars_per_word=100, lowercase=True,
                 strip_accents=None, clean_text=True, handle_chinese_chars=True, device=None):
        if isinstance(vocab, (str, bytes)) or not hasattr(vocab, "__iter__"):
            raise TypeError("vocab must be a list of str (one token per id), not %s" % type(vocab).__name__)
        vocab = list(vocab)
        for i, t in enumerate(vocab):
            if not isinstance(t, str):
                raise TypeError("vocab[%d] must be a str, not %s" % (i, type(t).__name__))
            if not t:
                raise ValueError("vocab[%d] is empty" % i)
        for name, v in (("unk_token", unk_token), ("continuing_subword_prefix", continuing_subword_prefix)):
            if not isinstance(v, str):
                raise TypeError("%s must be a str, not %s" % (name, type(v).__name__))
        if isinstance(max_input_chars_per_word, bool) or not isinstance(max_input_chars_per_word, int):
            raise TypeError("max_input_chars_per_word must be an int")
        if not 0 <= max_input_chars_per_word <= 1 << 20:
            raise ValueError("max_input_chars_per_word must lie in 0 .. 2**20")
        self._flags = _wp_tables.flags_of(lowercase, strip_accents, clean_text, handle_chinese_chars)
        if not vocab:
            raise ValueError("vocab is empty")
        if len(continuing_subword_prefix.encode("utf-8")) > 16:
            raise ValueError("continuing_subword_prefix is longer than 16 bytes")
        self._ids = {t: i for i, t in enumerate(vocab)}  # (the later id wins)
        if unk_token not in self._ids:
            raise ValueError("unk_token %r is not in the vocabulary" % (unk_token,))
        if "\x00" in unk_token or "\x00" in continuing_subword_prefix:
            raise ValueError("unk_token and continuing_subword_prefix must not hold U+0000")
        if device is not None and not isinstance(device, int) and not hasattr(device, "index"):
            raise TypeError("device must be a torch device, an int or None")
        self._vocab = vocab
        self.unk_token, self.continuing_subword_prefix = unk_token, continuing_subword_prefix
        self.max_input_chars_per_word = max_input_chars_per_word
        self._device = device
        self._handles = {}

    @classmethod
    def from_file(cls, path, **options):
        """A vocab.txt: one token a line, the id is the line number."""
        with open(path, "rb") as f:
            raw = f.read().decode("utf-8")
        lines = raw.split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        return cls([t[:-1] if t.endswith("\r") else t for t in lines], **options)

    @classmethod
    def from_tokenizer(cls, tok, device=None):
        """From a `tokenizers.Tokenizer` or a `transformers` fast tokenizer whose model is WordPiece behind a
        BertNormalizer and a BertPreTokenizer: their options and the vocabulary.  Anything else: ValueError."""
        from . import hf
        lines, options = hf.wordpiece_options(tok)
        return cls(lines, device=device, **options)

    @property
    def vocab_size(self):
        return len(self._vocab)

    def token_to_id(self, token):
        return self._ids.get(token)

    def id_to_token(self, i):
        return self._vocab[i] if 0 <= i < len(self._vocab) else None

    def _handle(self, dev):
        h = self._handles.get(dev.index)
        if h is None:
            strip = self._flags & _wp_tables.STRIP_ACCENTS
            h = self._handles[dev.index] = _capi.WordPiece(
                _wp_tables.table_blob(), _norm_tables.table_blob() if strip else None,
                [t.encode("utf-8", "surrogateescape") for t in self._vocab], self.unk_token.encode("utf-8"),
                self.continuing_subword_prefix.encode("utf-8"), self.max_input_chars_per_word, self._flags, dev.index)
        return h

    def encode_packed_device(self, d_bytes, d_offsets, check=True, return_word_ids=False):
        """Device tensors in (uint8 bytes, int64 offsets[n + 1]), device tensors out: (ids int32, out_offsets int64[n + 1])
        -- the pair every collate_* function and SequencePacker.add take -- and with return_word_ids the index of every
        id's word in its document (int32, what `tokenizers` calls word_ids; mask_tokens(word_ids=) takes it).  Runs on
        the current torch stream.  ids is a view of a buffer of the capacity bound; its length is read from the device,
        which is the call's one synchronisation.  check=True: offsets that do not describe d_bytes raise ValueError."""
        _packed_text_args(d_bytes, d_offsets)
        import torch
        dev = d_bytes.device
        h = self._handle(dev)
        n_docs, n_bytes = d_offsets.numel() - 1, d_bytes.numel()
        cap = h.ids_capacity(n_bytes, n_docs)

        def call():
            ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            oo = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
            wi = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_word_ids else None
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            h.batch_device(d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, ids.data_ptr(), cap, oo.data_ptr(),
                           wi.data_ptr() if return_word_ids else 0, err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return (ids, oo, err, wi) if return_word_ids else (ids, oo, err)

        res = _on_torch_stream(dev, call, used=(d_bytes, d_offsets))
        ids, oo, err = res[:3]
        code = int(err.item()) if check else 0
        if code:
            raise ValueError("hutoken_amd: WordPiece.encode_packed_device: device-side error %d (offsets that do not "
                             "describe d_bytes)" % code)
        total = int(oo[n_docs].item())
        return (ids[:total], oo, res[3][:total]) if return_word_ids else (ids[:total], oo)

    def batch_encode(self, texts):
        """A list of str -> a list of lists of ids, encoded on the GPU."""
        import numpy as np
        import torch
        if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
            raise TypeError("Invalid arguments. Expected a list of strings.")
        chunks = [t.encode("utf-8", "surrogateescape") for t in texts]
        offs = np.zeros(len(chunks) + 1, dtype=np.int64)
        if chunks:
            np.cumsum(np.fromiter(map(len, chunks), dtype=np.int64, count=len(chunks)), out=offs[1:])
        d = self._device
        dev = torch.device("cuda", torch.cuda.current_device() if d is None else d if isinstance(d, int) else
                           (d.index if d.index is not None else torch.cuda.current_device()))
        d_bytes = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()).to(dev)
        ids, oo = self.encode_packed_device(d_bytes, torch.from_numpy(offs).to(dev))
        flat, bounds = ids.tolist(), oo.tolist()
        return [flat[bounds[i]:bounds[i + 1]] for i in range(len(chunks))]

    def encode(self, text):
        """One str -> its list of ids."""
        if not isinstance(text, str):
            raise TypeError("Invalid arguments. Expected a string.")
        return self.batch_encode([text])[0]


# ---- Unigram (hutk_unigram.hip) ----
class Unigram:
    """A Unigram vocabulary (SentencePiece's language model: T5, mT5, ALBERT, XLNet, XLM-R, mBART, Pegasus) behind a
    Metaspace word split, encoding on the GPU what the `tokenizers` package encodes with models.Unigram(vocab, unk_id,
    byte_fallback=False) behind pre_tokenizers.Metaspace -- id for id and word id for word id.

    vocab: the (piece, score) pairs in id order (of two equal pieces the later id, with its own score, is found); unk_id
    is required.  prepend_scheme: "always" ("first" is read as "always") or "never".  whitespace_split=True is T5's
    shape, Sequence[WhitespaceSplit, Metaspace]; it needs prepend_scheme "always".  collapse_spaces=True is the
    normaliser step Replace(" {2,}", " ") of XLM-R and ALBERT.  device: a torch device, an index, or None for the
    current one; the table is uploaded at the first call that needs the GPU, once.  Needs no initialised context.

    Left out: SentencePiece's precompiled normaliser (nmt_nfkc and its kin), byte_fallback, sampling and n-best, decoding,
    token spans over the source text, special strings inside text, and binary .model files."""

    def __init__(self, vocab, unk_id, *, prepend_scheme="always", whitespace_split=False, collapse_spaces=False, device=None):
        import math
        if isinstance(vocab, (str, bytes, dict)) or not hasattr(vocab, "__iter__"):
            raise TypeError("vocab must be a list of (piece, score) pairs in id order, not %s" % type(vocab).__name__)
        vocab = list(vocab)
        pieces, scores = [], []
        for i, entry in enumerate(vocab):
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise TypeError("vocab[%d] must be a (piece, score) pair" % i)
            t, sc = entry
            if not isinstance(t, str):
                raise TypeError("vocab[%d]: the piece must be a str, not %s" % (i, type(t).__name__))
            if isinstance(sc, bool) or not isinstance(sc, (int, float)):
                raise TypeError("vocab[%d]: the score must be a float, not %s" % (i, type(sc).__name__))
            if not t:
                raise ValueError("vocab[%d] is empty" % i)
            if not math.isfinite(sc):
                raise ValueError("vocab[%d]: the score is not finite" % i)
            if len(t.encode("utf-8", "surrogateescape")) - 2 * t.count("\u2581") > 256:
                raise ValueError("vocab[%d] is longer than 256 bytes" % i)
            pieces.append(t)
            scores.append(float(sc))
        if isinstance(unk_id, bool) or not isinstance(unk_id, int):
            raise TypeError("unk_id must be an int (the reference raises at the first unknown character without one; here it is required)")
        for name, v in (("whitespace_split", whitespace_split), ("collapse_spaces", collapse_spaces)):
            if not isinstance(v, bool):
                raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))
        if not isinstance(prepend_scheme, str):
            raise TypeError("prepend_scheme must be a str")
        if prepend_scheme not in ("always", "first", "never"):
            raise ValueError("prepend_scheme must be \"always\", \"first\" or \"never\", not %r" % (prepend_scheme,))
        if not pieces:
            raise ValueError("vocab is empty")
        if not 0 <= unk_id < len(pieces):
            raise ValueError("unk_id %d is no id of the vocabulary" % unk_id)
        if whitespace_split and prepend_scheme == "never":
            raise ValueError("whitespace_split needs prepend_scheme \"always\"")
        if device is not None and not isinstance(device, int) and (isinstance(device, str) or not hasattr(device, "index")):
            raise TypeError("device must be a torch device, an int or None")
        self._pieces, self._scores, self.unk_id = pieces, scores, unk_id
        self._ids = {t: i for i, t in enumerate(pieces)}  # (the later id wins)
        self.prepend_scheme, self.whitespace_split, self.collapse_spaces = prepend_scheme, whitespace_split, collapse_spaces
        self._flags = ((0 if prepend_scheme == "never" else _capi.UG_PREPEND) | (_capi.UG_WHITESPACE_SPLIT if whitespace_split else 0)
                       | (_capi.UG_COLLAPSE_SPACES if collapse_spaces else 0))
        self.normalize = None  # the default of the list forms' normalize= (from_tokenizer sets it)
        self._device = device
        self._handles = {}

    @classmethod
    def from_file(cls, path, **options):
        """A tokenizer.json-style JSON file: the whole file, or its "model" object (type "Unigram", vocab, unk_id)."""
        import json
        with open(path, "rb") as f:
            obj = json.loads(f.read().decode("utf-8"))
        model = obj.get("model", obj) if isinstance(obj, dict) else None
        if not isinstance(model, dict) or model.get("type", "Unigram") != "Unigram" or "vocab" not in model:
            raise ValueError("%s holds no Unigram model (an object with type \"Unigram\", vocab and unk_id)" % path)
        if model.get("byte_fallback"):
            raise ValueError("%s: byte_fallback is not supported" % path)
        if model.get("unk_id") is None:
            raise ValueError("%s: the model has no unk_id" % path)
        return cls([(p, s) for p, s in model["vocab"]], model["unk_id"], **options)

    @classmethod
    def from_tokenizer(cls, tok, assume_normalized=False, device=None):
        """From a `tokenizers.Tokenizer` or a `transformers` fast tokenizer whose model is Unigram behind a Metaspace
        pre-tokenizer (hf.unigram_options lists what is accepted).  Anything else: ValueError naming the step; with
        assume_normalized=True the normaliser steps that cannot be reproduced are dropped and the caller vouches for
        the text.  A normalisation form (NFC .. NFKD) becomes the instance's `normalize` default."""
        from . import hf
        vocab, options = hf.unigram_options(tok, assume_normalized=assume_normalized)
        form = options.pop("normalize")
        unk_id = options.pop("unk_id")
        self = cls(vocab, unk_id, device=device, **options)
        self.normalize = form
        return self

    @property
    def vocab_size(self):
        return len(self._pieces)

    def token_to_id(self, token):
        return self._ids.get(token)

    def id_to_token(self, i):
        return self._pieces[i] if 0 <= i < len(self._pieces) else None

    def _handle(self, dev):
        h = self._handles.get(dev.index)
        if h is None:
            h = self._handles[dev.index] = _capi.Unigram([t.encode("utf-8", "surrogateescape") for t in self._pieces], self._scores,
                                                         self.unk_id, self._flags, dev.index)
        return h

    def encode_packed_device(self, d_bytes, d_offsets, check=True, return_word_ids=False):
        """Device tensors in (uint8 bytes, int64 offsets[n + 1]), device tensors out: (ids int32, out_offsets int64[n + 1])
        -- the pair every collate_* function and SequencePacker.add take -- and with return_word_ids the index of every
        id's word in its document (int32, what `tokenizers` calls word_ids; mask_tokens(word_ids=) takes it).  Runs on
        the current torch stream.  ids is a view of a buffer of the capacity bound (n_bytes + n_docs); its length is read
        from the device, which is the call's one synchronisation.  check=True: offsets that do not describe d_bytes raise
        ValueError."""
        _packed_text_args(d_bytes, d_offsets)
        import torch
        dev = d_bytes.device
        h = self._handle(dev)
        n_docs, n_bytes = d_offsets.numel() - 1, d_bytes.numel()
        cap = h.ids_capacity(n_bytes, n_docs)

        def call():
            ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            oo = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
            wi = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_word_ids else None
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            h.batch_device(d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, ids.data_ptr(), cap, oo.data_ptr(),
                           wi.data_ptr() if return_word_ids else 0, err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return (ids, oo, err, wi) if return_word_ids else (ids, oo, err)

        res = _on_torch_stream(dev, call, used=(d_bytes, d_offsets))
        ids, oo, err = res[:3]
        code = int(err.item()) if check else 0
        if code:
            raise ValueError("hutoken_amd: Unigram.encode_packed_device: device-side error %d (offsets that do not "
                             "describe d_bytes)" % code)
        total = int(oo[n_docs].item())
        return (ids[:total], oo, res[3][:total]) if return_word_ids else (ids[:total], oo)

    def batch_encode(self, texts, normalize=None):
        """A list of str -> a list of lists of ids, encoded on the GPU.  normalize="NFC" (.. "NFKD"): the packed text is
        put into that form on the GPU first (None: the instance's default, which from_tokenizer sets)."""
        import numpy as np
        import torch
        from .normalize import form_index  # (by module name: after a reload of the package its attribute `normalize` is the function)
        form = self.normalize if normalize is None else normalize
        if form is not None:
            form_index(form)
        if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
            raise TypeError("Invalid arguments. Expected a list of strings.")
        chunks = [t.encode("utf-8", "surrogateescape") for t in texts]
        offs = np.zeros(len(chunks) + 1, dtype=np.int64)
        if chunks:
            np.cumsum(np.fromiter(map(len, chunks), dtype=np.int64, count=len(chunks)), out=offs[1:])
        d = self._device
        dev = torch.device("cuda", torch.cuda.current_device() if d is None else d if isinstance(d, int) else
                           (d.index if d.index is not None else torch.cuda.current_device()))
        d_bytes = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        if form is not None:
            with torch.cuda.device(dev):
                d_bytes, d_offs = normalize_packed_device(d_bytes, d_offs, form)
        ids, oo = self.encode_packed_device(d_bytes, d_offs)
        flat, bounds = ids.tolist(), oo.tolist()
        return [flat[bounds[i]:bounds[i + 1]] for i in range(len(chunks))]

    def encode(self, text, normalize=None):
        """One str -> its list of ids."""
        if not isinstance(text, str):
            raise TypeError("Invalid arguments. Expected a string.")
        return self.batch_encode([text], normalize=normalize)[0]


# ---- split presets (hutk_presplit.hip) ----
_pretokenizers = {}


def _pretokenizer(dev):
    """The pre-tokeniser of a torch device: its tables are built once per process and uploaded once per device."""
    pt = _pretokenizers.get(dev.index)
    if pt is None:
        pt = _pretokenizers[dev.index] = _capi.Pretokenizer(_presplit_tables.table_blob(), dev.index)
    return pt


def set_pretokenizer(name):
    """Install a split preset on the initialised context -- "gpt2", "cl100k" (alias "llama3"), "qwen2"; the patterns
    are hutoken_amd.pretokenize.PATTERNS -- or remove it with None.  Every encoder of the package then splits by it, on the
    GPU and with no host round trip: encode, batch_encode, the *_packed_device forms, SequencePacker.add_texts,
    batch_encode_with_offsets, the special-token functions.  The presets are for byte-level vocabularies: a context
    with a prefix, one with a regex pattern, and the byte-fallback functions refuse (RuntimeError, not supported)."""
    if _ctx is None:
        raise RuntimeError("Vocabulary is not initialized for encoding. Call 'initialize' function first.")
    if name is None:
        _ctx.set_pretokenizer(None)
    else:
        _ctx.set_pretokenizer(_presplit_tables.preset_index(name), _presplit_tables.table_blob())


def pretokenize_packed_device(d_bytes, d_offsets, preset, *, return_bits=False):
    """The word split of a preset -- "gpt2", "cl100k" (alias "llama3") or "qwen2", the patterns of
    hutoken_amd.pretokenize.PATTERNS -- of a packed batch on the GPU: device tensors in (uint8 bytes, int64 offsets[n+1],
    as encode_packed_device takes them), (starts, start_offsets) out: the ascending byte positions (int64, into d_bytes)
    at which a word starts, and int64[n+1] offsets into them, document i's words being starts[start_offsets[i] :
    start_offsets[i + 1]] (each ends where the next starts, the last at the document's end).  Per document this is
    [m.start() for m in regex.finditer(pattern, d.decode("utf-8", "surrogateescape"))] in bytes: a byte that strict
    UTF-8 rejects is one character that is neither letter, number nor whitespace; documents are independent; the
    classes are those of this interpreter's unicodedata.  d_bytes may be a view at any byte offset.

    Runs on the current torch stream: the split, a count, one synchronising read of the count (and the error word), the
    listing.  return_bits=True: the bitmap itself instead (int32[n_bytes // 32 + 40], bit p: a word starts at byte p,
    the bit at n_bytes set), enqueued without any synchronisation; offsets that do not describe d_bytes then leave it
    unwritten.  Otherwise they raise ValueError.  Needs no initialised context and touches no vocabulary."""
    pi = _presplit_tables.preset_index(preset)
    _packed_text_args(d_bytes, d_offsets)
    import torch
    dev = d_bytes.device
    pt = _pretokenizer(dev)
    n_docs, n_bytes = d_offsets.numel() - 1, d_bytes.numel()
    n_words = n_bytes // 32 + 1
    with torch.cuda.device(dev):
        bits = torch.empty(n_bytes // 32 + 40, dtype=torch.int32, device=dev)
        small = torch.zeros(2, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        pt.batch_device(pi, d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, bits.data_ptr(), small.data_ptr(), stream)
        if return_bits:
            return bits
        before = torch.zeros(n_words + 1, dtype=torch.int64, device=dev)
        pt.starts_device(bits.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, before.data_ptr(), 0, 0, stream)
        code = int(small[0])  # the one synchronisation
        if code:
            raise ValueError("hutoken_amd: pretokenize_packed_device: device-side error %d (offsets that do not describe d_bytes)" % code)
        total = int(before[n_words]) - 1
        starts = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        start_offs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        pt.starts_device(bits.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, before.data_ptr(), starts.data_ptr(),
                         start_offs.data_ptr(), stream)
    return starts[:total], start_offs


def pretokenize(texts, preset):
    """A list of str -> for each the list of its words under the preset ("gpt2", "cl100k" / "llama3", "qwen2"), what
    pre_tokenize_str gives elsewhere, split on the current GPU (pretokenize_packed_device; no context is needed).  The
    words of a text concatenate to it."""
    import numpy as np
    import torch
    _presplit_tables.preset_index(preset)
    if not isinstance(texts, list):
        raise TypeError("Invalid arguments. Expected a list of strings.")
    try:
        chunks = [t.encode("utf-8", "surrogateescape") for t in texts]
    except AttributeError:
        raise TypeError("Invalid arguments. Expected a list of strings.")
    offs = np.zeros(len(chunks) + 1, dtype=np.int64)
    if chunks:
        np.cumsum(np.fromiter(map(len, chunks), dtype=np.int64, count=len(chunks)), out=offs[1:])
    dev = torch.device("cuda", torch.cuda.current_device())
    raw = b"".join(chunks)
    d_bytes = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
    starts, so = pretokenize_packed_device(d_bytes, torch.from_numpy(offs).to(dev), preset)
    starts, so = starts.tolist(), so.tolist()
    out = []
    for i in range(len(chunks)):
        edges = starts[so[i]:so[i + 1]] + [int(offs[i + 1])]
        out.append([raw[a:b].decode("utf-8", "surrogateescape") for a, b in zip(edges, edges[1:])])
    return out


# ---- row-aligned features: the gather, word ids, answer positions -----------------------------------------
_NO_PRESET = ("word ids need a split preset (set_pretokenizer, or preset=): the built-in splitter's word starts are not on "
              "the device as a bitmap")


def _is_tensor(t):
    return hasattr(t, "data_ptr") and hasattr(t, "is_cuda") and hasattr(t, "dtype")


def _dtype_name(t):
    return str(t.dtype).rpartition(".")[2]


def _plan_arg(row_plan):
    if not _is_tensor(row_plan):
        raise TypeError("row_plan must be a torch tensor, not %s" % type(row_plan).__name__)
    if _dtype_name(row_plan) != "int64":
        raise TypeError("row_plan must have dtype int64, not %s" % row_plan.dtype)
    if row_plan.dim() != 2 or row_plan.shape[1] != 8 or not row_plan.is_contiguous():
        raise ValueError("row_plan must be contiguous and of shape [n_rows, 8]")


def _records_arg(name, t, pairs_only=False):
    """A per-token array: [n] or [n, 2], int32 or int64, contiguous -> (dtype name, record bytes)."""
    if not _is_tensor(t):
        raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
    dname = _dtype_name(t)
    if dname not in ("int32", "int64"):
        raise TypeError("%s must have dtype int32 or int64, not %s" % (name, t.dtype))
    shape_ok = (t.dim() == 2 and t.shape[1] == 2) or (t.dim() == 1 and not pairs_only)
    if not shape_ok or not t.is_contiguous():
        raise ValueError("%s must be contiguous and of shape %s[n, 2]" % (name, "" if pairs_only else "[n] or "))
    return dname, (4 if dname == "int32" else 8) * (2 if t.dim() == 2 else 1)


def _fill_arg(fill, per, dname):
    """fill -> the record as bytes: an int, or with records of two values a pair of ints (an int then fills both)."""
    import struct
    vals = tuple(fill) if isinstance(fill, (tuple, list)) else (fill,)
    if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
        raise TypeError("fill must be an int or a pair of ints")
    if len(vals) not in (1, per):
        raise ValueError("fill must be an int%s, not %d values" % (" or a pair of ints" if per == 2 else "", len(vals)))
    bits = 31 if dname == "int32" else 63
    if any(not -2**bits <= v < 2**bits for v in vals):
        raise ValueError("fill must fit %s" % dname)
    return struct.pack("<%d%s" % (per, "i" if dname == "int32" else "q"), *(vals * per if len(vals) == 1 else vals))


def gather_rows(row_plan, max_length, values_a, values_b=None, *, fill=0, check=False):
    """Any per-token array in the rows' shape: row_plan int64 [n_rows, 8] (return_plan=True of a collate_* call made with
    this max_length) and values_a, a device tensor [n] or [n, 2] of int32 or int64 indexed like that call's ids_a (spans,
    word ids, labels) -> [n_rows, max_length] or [n_rows, max_length, 2] of the same dtype: the value of the token a
    column holds, `fill` (an int, or a pair of ints for [n, 2]) where it holds bos, a separator, eos or padding.
    values_b: the B side's array, like ids_b; None reads both sides from values_a -- the one-encode-call case of
    batch_encode_pairs.  On the current torch stream, never synchronises; check=True does and raises ValueError for a
    plan that points outside the row or the values (nothing is read or written out of bounds either way)."""
    _plan_arg(row_plan)
    _length_arg("max_length", max_length, 1)
    dname, rec = _records_arg("values_a", values_a)
    if values_b is not None and (_records_arg("values_b", values_b) != (dname, rec)):
        raise TypeError("values_b must have the dtype and the record shape of values_a")
    per = 2 if values_a.dim() == 2 else 1
    fill_bytes = _fill_arg(fill, per, dname)
    vb = values_a if values_b is None else values_b
    for name, t in (("row_plan", row_plan), ("values_a", values_a), ("values_b", vb)):
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU: the gather runs there and nowhere else" % name)
        if t.device != row_plan.device:
            raise ValueError("%s must be on the device of row_plan" % name)
    import torch
    dev = row_plan.device
    n_rows = row_plan.shape[0]
    out = torch.empty((n_rows, max_length) + ((2,) if per == 2 else ()), dtype=values_a.dtype, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.rows_gather_device(row_plan.data_ptr(), n_rows, max_length, values_a.data_ptr(), values_a.shape[0],
                                 vb.data_ptr(), vb.shape[0], rec, fill_bytes, out.data_ptr(), err.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
        return out
    _on_torch_stream(dev, call, used=(row_plan, values_a, vb, err))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: gather_rows: a row_plan that points outside its row or the values (device-side "
                         "error %d)" % int(err.item()))
    return out


def answer_positions(row_plan, spans, answers, *, side="b", check=False):
    """The columns at which an answer starts and ends in every row, for extractive QA: row_plan int64 [n_rows, 8], spans
    [n, 2] (int32 or int64) of the tokens of `side` ("a" or "b"; indexed like that side's ids, e.g. token_spans_device
    of the one encode call), answers [n_items, 2] with (start, end) of item i's answer in the spans' unit, from the start
    of that side's text, (-1, -1) or start >= end for none -> int32 [n_rows, 2].  An answer lies in a row when the row's
    tokens of that side cover it: the start column is that of the last token starting at or before `start`, the end
    column that of the first token ending at or after `end` (run_qa's rule, on the window's own tokens); a row that
    does not hold the whole answer gets (-1, -1), which the caller maps to its CLS column.  On the current torch stream,
    never synchronises; check=True does and raises ValueError for a plan that points outside spans or answers."""
    _plan_arg(row_plan)
    dname, rec = _records_arg("spans", spans, pairs_only=True)
    _records_arg("answers", answers, pairs_only=True)
    if side not in ("a", "b"):
        raise ValueError("side must be 'a' or 'b', not %r" % (side,))
    for name, t in (("row_plan", row_plan), ("spans", spans), ("answers", answers)):
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU: the search runs there and nowhere else" % name)
        if t.device != row_plan.device:
            raise ValueError("%s must be on the device of row_plan" % name)
    import torch
    dev = row_plan.device
    n_rows = row_plan.shape[0]
    ans = answers if answers.dtype == spans.dtype else answers.to(spans.dtype)
    out = torch.empty((n_rows, 2), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.rows_answers_device(row_plan.data_ptr(), n_rows, 1 if side == "b" else 0, spans.data_ptr(), rec // 2,
                                  spans.shape[0], ans.data_ptr(), ans.shape[0], out.data_ptr(), err.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
        return out
    _on_torch_stream(dev, call, used=(row_plan, spans, ans, err))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: answer_positions: a row_plan that points outside spans or answers (device-side "
                         "error %d)" % int(err.item()))
    return out


def token_word_ids_device(d_bytes, d_offsets, ids, out_offsets, *, preset=None, n_ids=None, check=True):
    """The packed text and what encode_packed_device made of it (as token_spans_device takes them) -> a device tensor
    int32 [n_ids]: the word of its document each token starts in, counted from 0 -- what word_ids() gives elsewhere,
    for aligning word-level labels (NER, POS) to tokens.  The words are those of a split preset ("gpt2", "cl100k" /
    "llama3", "qwen2"); preset=None uses the one installed on the context (set_pretokenizer).  A context without one and
    no preset= raises ValueError: the built-in splitter's word starts are not on the device as a bitmap, so there is
    nothing to rank the tokens in.  Runs the split's bitmap, its prefix counts, the byte spans (token_spans_device) and
    the rank kernel on the current torch stream.  check=True synchronises and raises as token_spans_device does, and
    ValueError naming the first document that has a token with a word start strictly inside it: its ids were made
    under another split (the other documents' word ids are exact)."""
    if _ctx is None:
        raise RuntimeError(_NOT_INIT)
    if preset is None:
        pi = _ctx.pretokenizer
        if pi is None:
            raise ValueError(_NO_PRESET)
    else:
        pi = _presplit_tables.preset_index(preset)
    spans = token_spans_device(d_bytes, d_offsets, ids, out_offsets, unit="byte", n_ids=n_ids, check=check)
    import torch
    dev = ids.device
    n_docs, n_bytes, n_ids = d_offsets.numel() - 1, d_bytes.numel(), spans.shape[0]
    pt = _pretokenizer(dev)
    words = torch.empty(n_ids, dtype=torch.int32, device=dev)
    bits = torch.empty(n_bytes // 32 + 40, dtype=torch.int32, device=dev)
    before = torch.zeros(n_bytes // 32 + 2, dtype=torch.int64, device=dev)
    status = torch.zeros(max(n_docs, 1), dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)  # one word per call

    def call():
        stream = torch.cuda.current_stream(dev).cuda_stream
        pt.batch_device(pi, d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, bits.data_ptr(), err[0:].data_ptr(), stream)
        pt.starts_device(bits.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, before.data_ptr(), 0, 0, stream)
        _capi.token_word_ids_device(bits.data_ptr(), before.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes,
                                    spans.data_ptr(), 4, out_offsets.data_ptr(), n_ids, words.data_ptr(), status.data_ptr(),
                                    err[1:].data_ptr(), stream)
        return words
    _on_torch_stream(dev, call, used=(d_bytes, d_offsets, out_offsets, spans, bits, before, status, err))
    if check:
        codes = err.tolist()
        if codes[0] or codes[1] == _capi.E_ARG:
            raise TypeError("hutoken_amd: token_word_ids_device: offsets that do not describe the tensors")
        if codes[1]:
            which = int(torch.nonzero(status[:n_docs]).flatten()[0].item())
            raise ValueError("hutoken_amd: token_word_ids_device: document %d: a token holds a word start of the %s split "
                             "strictly inside it: the ids were made under another split (device-side error %d)"
                             % (which, _presplit_tables.PRESETS[pi], codes[1]))
    return words


# ---- targets: masked-LM corruption and loss labels ---------------------------------------------------------
_MLM_SIDES = {"a": _capi.MLM_SIDE_A, "b": _capi.MLM_SIDE_B, "both": _capi.MLM_SIDE_A | _capi.MLM_SIDE_B}
_LOSS_ON = {"a": _capi.LABELS_A, "b": _capi.LABELS_B, "template": _capi.LABELS_TEMPLATE, "end": _capi.LABELS_END}


def _rows_arg(name, t):
    """input_ids of rows: [n_rows, L] with L >= 1, int32 or int64, contiguous -> (dtype name, element bytes)."""
    if not _is_tensor(t):
        raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
    dname = _dtype_name(t)
    if dname not in ("int32", "int64"):
        raise TypeError("%s must have dtype int32 or int64, not %s" % (name, t.dtype))
    if t.dim() != 2 or t.shape[1] < 1 or not t.is_contiguous():
        raise ValueError("%s must be contiguous and of shape [n_rows, L] with L >= 1" % name)
    _length_arg("the row length of %s" % name, t.shape[1], 1)
    return dname, 4 if dname == "int32" else 8


def _rows_plan_arg(row_plan, input_ids):
    _plan_arg(row_plan)
    if row_plan.shape[0] != input_ids.shape[0]:
        raise ValueError("row_plan must hold one row for every row of input_ids (%d), not %d" % (input_ids.shape[0], row_plan.shape[0]))


def _fraction_arg(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s must be a number in [0, 1], not %s" % (name, type(v).__name__))
    if not 0 <= v <= 1:  # (NaN is refused too)
        raise ValueError("%s must be in [0, 1], not %r" % (name, v))
    return float(v)


def _ignore_arg(ignore_index, dname):
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise TypeError("ignore_index must be an int, not %s" % type(ignore_index).__name__)
    bits = 31 if dname == "int32" else 63
    if not -2**bits <= ignore_index < 2**bits:
        raise ValueError("ignore_index must fit %s" % dname)
    return ignore_index


def _on_one_gpu(what, named):
    """named: (name, tensor) -- all on the GPU and on the device of the first"""
    for name, t in named:
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU: %s runs there and nowhere else" % (name, what))
        if t.device != named[0][1].device:
            raise ValueError("%s must be on the device of %s" % (name, named[0][0]))


def _seed_arg(seed):
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError("seed must be an int, not %s" % type(seed).__name__)
    if not 0 <= seed < 2**64:
        raise ValueError("seed must be in 0 .. 2**64 - 1, not %d" % seed)
    return seed


def _mlm_args(mask_id, vocab_size, seed, mlm_probability, mask_fraction, random_fraction):
    """What mask_tokens checks of its numbers -> (mask_id, vocab_size, select_below, mask_below, random_below): a
    probability p is the threshold int(p * 2**32) against a draw of 32 bits."""
    mask_id = _token_arg("mask_id", mask_id, False)
    p_select = _fraction_arg("mlm_probability", mlm_probability)
    p_mask, p_random = _fraction_arg("mask_fraction", mask_fraction), _fraction_arg("random_fraction", random_fraction)
    if p_mask + p_random > 1 + 1e-12:
        raise ValueError("mask_fraction + random_fraction must not be above 1, not %r" % (p_mask + p_random,))
    if vocab_size is None:
        if p_random != 0:
            raise ValueError("vocab_size=None is allowed only with random_fraction == 0")
    elif isinstance(vocab_size, bool) or not isinstance(vocab_size, int):
        raise TypeError("vocab_size must be an int or None, not %s" % type(vocab_size).__name__)
    elif not 1 <= vocab_size <= 2**31:
        raise ValueError("vocab_size must be in 1 .. 2**31, not %d" % vocab_size)
    _seed_arg(seed)
    mask_below = int(p_mask * 2**32)
    random_below = min(2**32, max(mask_below, int((p_mask + p_random) * 2**32)))
    return mask_id, 1 if vocab_size is None else vocab_size, int(p_select * 2**32), mask_below, random_below


def mask_tokens(input_ids, row_plan, *, mask_id, vocab_size=None, seed, mlm_probability=0.15, mask_fraction=0.8,
                random_fraction=0.1, word_ids=None, word_ids_b=None, sides="both", ignore_index=-100, inplace=False,
                check=False):
    """The masked-LM corruption of collated rows, one HIP pass: input_ids [n_rows, L] int32 or int64 on the GPU and the
    row_plan of the collate_* call that made them -> (input_ids, labels), both of input_ids' shape and dtype.  Only the
    columns that hold a token of a text (of side "a", "b" or "both": `sides`) can be selected -- never bos, a separator,
    eos or padding.  A selected column keeps its id in labels and becomes mask_id with probability mask_fraction, a
    random id below vocab_size with random_fraction, and stays otherwise; every other column is copied and gets
    ignore_index.  vocab_size=None is allowed only with random_fraction == 0.  Token mode selects every eligible column
    with mlm_probability; with word_ids (the flat int32 tensor of token_word_ids_device for the encode call the rows
    were made from; word_ids_b: the B side's, None reads both sides from word_ids) every word is selected with
    mlm_probability and all its tokens in the row with it, and a token whose word id is below 0 is protected.
    The random numbers are Philox4x32-10 draws that depend on nothing but (seed, row, column) or (seed, row, side, word)
    -- include/hutoken_amd.h states the rule in full, tests/targets_ref.py restates it in numpy -- so a row's outcome
    does not depend on the batch around it, and the same seed gives the same result anywhere.  seed is an int in
    0 .. 2**64 - 1 and has no default: there is no hidden state; pass a different one per step.  A probability p is the
    threshold int(p * 2**32) against a draw of 32 bits.  inplace=True overwrites input_ids and returns it.  On the
    current torch stream, never synchronises; check=True does and raises ValueError for a plan that points outside its
    row or the word ids (nothing is read or written out of bounds either way)."""
    dname, width = _rows_arg("input_ids", input_ids)
    _rows_plan_arg(row_plan, input_ids)
    mask_id, vocab, select_below, mask_below, random_below = _mlm_args(mask_id, vocab_size, seed, mlm_probability, mask_fraction,
                                                                       random_fraction)
    if sides not in _MLM_SIDES:
        raise ValueError("sides must be 'a', 'b' or 'both', not %r" % (sides,))
    _ignore_arg(ignore_index, dname)
    if not isinstance(inplace, bool):
        raise TypeError("inplace must be a bool, not %s" % type(inplace).__name__)
    if word_ids is None and word_ids_b is not None:
        raise ValueError("word_ids_b needs word_ids")
    named = [("input_ids", input_ids), ("row_plan", row_plan)]
    for name, t in (("word_ids", word_ids), ("word_ids_b", word_ids_b)):
        if t is None:
            continue
        if not _is_tensor(t):
            raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
        if _dtype_name(t) != "int32":
            raise TypeError("%s must have dtype int32, not %s" % (name, t.dtype))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be one-dimensional and contiguous" % name)
        named.append((name, t))
    _on_one_gpu("the corruption", named)
    import torch
    dev = input_ids.device
    n_rows, L = input_ids.shape
    out = input_ids if inplace else torch.empty_like(input_ids)
    labels = torch.empty_like(input_ids)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    wa, wb = word_ids, word_ids_b
    if wa is not None and wa.numel() == 0:  # (an empty tensor has no address, and no address means token mode)
        wa = torch.zeros(1, dtype=torch.int32, device=dev)
    n_a = 0 if word_ids is None else word_ids.numel()

    def call():
        _capi.rows_mlm_device(row_plan.data_ptr(), n_rows, L, input_ids.data_ptr(), width,
                              0 if wa is None else wa.data_ptr(), n_a,
                              0 if wb is None or wb.numel() == 0 else wb.data_ptr(), 0 if wb is None else wb.numel(),
                              seed, select_below, mask_below, random_below, mask_id, vocab,
                              ignore_index, _MLM_SIDES[sides], out.data_ptr(), labels.data_ptr(), err.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
        return out, labels
    _on_torch_stream(dev, call, used=tuple(t for _n, t in named) + (err,) + (() if wa is None else (wa,)))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: mask_tokens: a row_plan that points outside its row or the word ids (device-side "
                         "error %d)" % int(err.item()))
    return out, labels


def _loss_on_arg(loss_on):
    if loss_on == "all":
        return sum(_LOSS_ON.values())
    if loss_on == "completion":
        return _capi.LABELS_B | _capi.LABELS_END
    if isinstance(loss_on, (tuple, list)) and loss_on and all(isinstance(x, str) and x in _LOSS_ON for x in loss_on):
        flags = 0
        for x in loss_on:
            flags |= _LOSS_ON[x]
        return flags
    raise ValueError("loss_on must be 'all', 'completion' or a non-empty tuple drawn from ('a', 'b', 'template', 'end'), "
                     "not %r" % (loss_on,))


def lm_labels(input_ids, attention_mask, row_plan, *, loss_on="all", shift=False, ignore_index=-100, check=False):
    """The loss labels of collated rows, one HIP pass: input_ids [n_rows, L] int32 or int64, attention_mask uint8 of the
    same shape and the row_plan of the collate_* call that made them -> labels of input_ids' shape and dtype: the id on
    the columns that carry loss, ignore_index on the others.  Padding never carries loss.  loss_on="all": every real
    column; "completion": the B side and eos -- SFT on batch_encode_pairs(prompts, answers, ...), where the prompt, bos
    and the separators carry none; or a tuple drawn from ("a", "b", "template", "end"), template being bos and the
    separators, end being eos.  shift=True gives labels[r][c] = what column c predicts: the id of column c + 1 when that
    one carries loss and column c is real, ignore_index otherwise (the last column predicts nothing) -- for a loss
    that does not shift by itself.  On the current torch stream, never synchronises; check=True does and raises
    ValueError for a plan that points outside its row."""
    dname, width = _rows_arg("input_ids", input_ids)
    if not _is_tensor(attention_mask):
        raise TypeError("attention_mask must be a torch tensor, not %s" % type(attention_mask).__name__)
    if _dtype_name(attention_mask) != "uint8":
        raise TypeError("attention_mask must have dtype uint8, not %s" % attention_mask.dtype)
    if tuple(attention_mask.shape) != tuple(input_ids.shape) or not attention_mask.is_contiguous():
        raise ValueError("attention_mask must be contiguous and of the shape of input_ids")
    _rows_plan_arg(row_plan, input_ids)
    flags = _loss_on_arg(loss_on)
    if not isinstance(shift, bool):
        raise TypeError("shift must be a bool, not %s" % type(shift).__name__)
    _ignore_arg(ignore_index, dname)
    _on_one_gpu("the labelling", (("input_ids", input_ids), ("attention_mask", attention_mask), ("row_plan", row_plan)))
    import torch
    dev = input_ids.device
    n_rows, L = input_ids.shape
    labels = torch.empty_like(input_ids)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.rows_labels_device(row_plan.data_ptr(), n_rows, L, input_ids.data_ptr(), width, attention_mask.data_ptr(),
                                 flags | (_capi.LABELS_SHIFT if shift else 0), ignore_index, labels.data_ptr(),
                                 err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return labels
    _on_torch_stream(dev, call, used=(input_ids, attention_mask, row_plan, err))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: lm_labels: a row_plan that points outside its row (device-side error %d)"
                         % int(err.item()))
    return labels


def _segments_arg(segment_ids):
    """segment_ids of packed rows: int32 [n_rows, L] with L >= 1, contiguous."""
    if not _is_tensor(segment_ids):
        raise TypeError("segment_ids must be a torch tensor, not %s" % type(segment_ids).__name__)
    if _dtype_name(segment_ids) != "int32":
        raise TypeError("segment_ids must have dtype int32, not %s" % segment_ids.dtype)
    if segment_ids.dim() != 2 or segment_ids.shape[1] < 1 or not segment_ids.is_contiguous():
        raise ValueError("segment_ids must be contiguous and of shape [n_rows, L] with L >= 1")


def packed_cu_seqlens(segment_ids, *, cap=None, check=False):
    """cu_seqlens for varlen attention from the segment_ids of packed rows (SequencePacker.add, .flush, or both
    concatenated), one stream compaction in HIP: segment_ids int32 [n_rows, L] -> (cu_seqlens int32 [cap + 1],
    info int32 [2] = (n_seq, max_seqlen), both on the device).  Flat element r * L + c starts a sequence when c == 0 or
    its segment differs from the one before it in the row, so the sequences are the pieces of documents in each row and
    a padding run is one of its own (its labels are ignore_index).  cu_seqlens holds the rising starts and then
    n_rows * L in every remaining slot: the surplus sequences have length zero.  With a given `cap` the call never
    synchronises; cap below n_seq writes the first cap starts, info[0] still holds
    the true count, and check=True raises ValueError naming both.  cap=None reads the count once -- the one
    synchronisation -- and returns cu_seqlens of exactly n_seq + 1 entries.  On the current torch stream."""
    _segments_arg(segment_ids)
    if cap is not None:
        if isinstance(cap, bool) or not isinstance(cap, int):
            raise TypeError("cap must be an int or None, not %s" % type(cap).__name__)
        if cap < 0 or cap >= _INT32_MAX:
            raise ValueError("cap must be in 0 .. 2**31 - 2")
    n_rows, L = segment_ids.shape
    if n_rows * L > _INT32_MAX:
        raise ValueError("segment_ids must hold fewer than 2**31 elements: cu_seqlens is int32")
    if not segment_ids.is_cuda:
        raise ValueError("segment_ids must be on the GPU: packed_cu_seqlens runs there and nowhere else")
    import torch
    dev = segment_ids.device
    room = n_rows * L if cap is None else cap  # (no more sequences than elements)
    cu = torch.empty(room + 1, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.packed_cu_seqlens_device(segment_ids.data_ptr(), n_rows, L, room, cu.data_ptr(), info.data_ptr(),
                                       err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return cu, info
    _on_torch_stream(dev, call, used=(segment_ids, err))
    if cap is None:
        return cu[:int(info[0].item()) + 1], info
    if check and int(err.item()):
        raise ValueError("hutoken_amd: packed_cu_seqlens: cap = %d is below the %d sequences of the rows" % (cap, int(info[0].item())))
    return cu, info


def packed_lm_labels(values, segment_ids, *, shift=False, ignore_index=-100):
    """The loss labels of packed rows, one HIP pass: values [n_rows, L] int32 or int64 -- the rows' input_ids for plain
    causal LM, or a packed `labels` channel (SequencePacker(channels=...)) where everything off the assistant's turns is
    ignore_index already -- and the rows' segment_ids -> labels of values' shape and dtype.  shift=False: the value on
    every real column (segment != 0), ignore_index on padding.  shift=True: what column c predicts, values[r][c + 1], when
    column c + 1 is in the row and of the same, real segment; ignore_index otherwise, so that no column predicts across
    a document boundary, a row end or into padding -- lm_labels(shift=True) for the packed layout.  On the current torch
    stream, never synchronises."""
    dname, width = _rows_arg("values", values)
    _segments_arg(segment_ids)
    if tuple(segment_ids.shape) != tuple(values.shape):
        raise ValueError("segment_ids must be of the shape of values")
    if not isinstance(shift, bool):
        raise TypeError("shift must be a bool, not %s" % type(shift).__name__)
    _ignore_arg(ignore_index, dname)
    _on_one_gpu("the labelling", (("values", values), ("segment_ids", segment_ids)))
    import torch
    dev = values.device
    n_rows, L = values.shape
    labels = torch.empty_like(values)

    def call():
        _capi.packed_labels_device(values.data_ptr(), width, segment_ids.data_ptr(), n_rows, L, shift, ignore_index,
                                   labels.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return labels
    _on_torch_stream(dev, call, used=(values, segment_ids))
    return labels


def pack_best_fit(ids, offsets, seq_len, *, bos_id=None, eos_id=None, pad_id=0, dtype=None, n_ids=None, n_rows=None,
                  check=False, return_source=False, return_doc_map=False):
    """Device tensors of encode_packed_device in, rows of WHOLE documents out, on the current torch stream (Ding et al.
    2024, "Fewer Truncations Improve Language Modeling"): -> dict of input_ids [n_rows, seq_len] of `dtype` (torch.int32,
    the default, or torch.int64), position_ids and segment_ids int32 [n_rows, seq_len], lengths int32 [n_rows] (the filled
    columns) and, on request, source int64 [n_rows, seq_len] -- the index into ids of the token at that element, -1 for
    bos, eos and padding: what gather_source takes -- and doc_map int64 [n_docs, 4] = (whole_row, n_whole, row, col).
    Document i's sequence is [bos_id] + its ids + [eos_id] (those given).  Only a sequence longer than seq_len is cut:
    every seq_len tokens of it are a row of their own (the first rows of the result, in document order, segment 1), and
    what remains of it, like every shorter sequence, is an item.  The items are packed best-fit-decreasing: taken by
    (length descending, document ascending), each into the open row with the least room that still holds it (the lowest
    such row), else into a new row.  Inside a row segment_ids count the items 1, 2, .. and are 0 on the padding behind
    the last one; position_ids restart at 0 with every item (SequencePacker's rule), so packed_lm_labels and
    packed_cu_seqlens take these rows as they are.  A call packs what it is given: nothing is carried to the next one.
    n_rows=None reads the number of rows once -- the one synchronisation (and one more for offsets[-1] without n_ids=);
    a given n_rows is the capacity of the result and the call then reads nothing back: rows behind the last real one are
    padding with length 0, and a capacity below the number of rows is a device-side error.  (The kernels' scratch is one
    buffer per device; a call that needs more of it than any call before waits for the device once, before its first
    kernel, while the buffer grows.)  check=True synchronises and raises
    ValueError on such an error (7: n_rows is too small; 4: offsets that do not describe ids).  seq_len above 65536 is
    refused."""
    bos, eos, pad = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
    s = (bos != _capi.NO_TOKEN) + (eos != _capi.NO_TOKEN)
    _length_arg("seq_len", seq_len, max(1, s))
    if seq_len > 65536:
        raise ValueError("seq_len must be at most 65536 for best-fit packing")
    width, dname = _out_width(dtype)
    _n_rows_arg(n_rows)
    _ragged_args(ids, offsets, n_ids)
    import torch
    dev = ids.device
    n_docs = offsets.numel() - 1
    n_ids = _n_ids(ids, offsets, n_ids)
    doc_map = torch.empty((n_docs, 4), dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    err = torch.zeros(2, dtype=torch.int32, device=dev)  # one word per call

    def call():
        stream = torch.cuda.current_stream(dev).cuda_stream
        cap = n_rows
        if cap is None:
            bound = _capi.bestfit_rows_bound(n_docs, n_ids, seq_len, s)
            _capi.bestfit_plan_device(offsets.data_ptr(), n_docs, n_ids, seq_len, bos, eos, bound, doc_map.data_ptr(),
                                      info.data_ptr(), err[0:].data_ptr(), stream)
            cap = int(info[0].item())  # the one synchronisation; pass n_rows= to avoid it
            if cap < 0 or cap > bound:
                raise ValueError("hutoken_amd: pack_best_fit: offsets that do not describe ids (%d rows)" % cap)
        else:
            _capi.bestfit_plan_device(offsets.data_ptr(), n_docs, n_ids, seq_len, bos, eos, cap, doc_map.data_ptr(),
                                      info.data_ptr(), err[0:].data_ptr(), stream)
        out = torch.empty((cap, seq_len), dtype=getattr(torch, dname), device=dev)
        pos = torch.empty((cap, seq_len), dtype=torch.int32, device=dev)
        seg = torch.empty((cap, seq_len), dtype=torch.int32, device=dev)
        lengths = torch.empty(cap, dtype=torch.int32, device=dev)
        source = torch.empty((cap, seq_len), dtype=torch.int64, device=dev) if return_source else None
        _capi.bestfit_rows_device(ids.data_ptr(), offsets.data_ptr(), doc_map.data_ptr(), n_docs, n_ids, seq_len, bos, eos,
                                  pad, width, cap, out.data_ptr(), pos.data_ptr(), seg.data_ptr(), lengths.data_ptr(),
                                  0 if source is None else source.data_ptr(), err[1:].data_ptr(), stream)
        return (out, pos, seg, lengths) + (() if source is None else (source,))
    res = _on_torch_stream(dev, call, used=(ids, offsets, doc_map, info, err))
    if check:
        codes = err.tolist()
        if codes[0] or codes[1]:
            raise ValueError("hutoken_amd: pack_best_fit: device-side error %d (7: n_rows is below the number of rows; 4: "
                             "offsets that do not describe ids)" % (codes[0] or codes[1]))
    out = {"input_ids": res[0], "position_ids": res[1], "segment_ids": res[2], "lengths": res[3]}
    if return_source:
        out["source"] = res[4]
    if return_doc_map:
        out["doc_map"] = doc_map
    return out


def gather_source(source, values, fill, *, check=False):
    """Any per-token array along a `source` array: source int64 of any shape (pack_best_fit(return_source=True), the
    chat render's or fill-in-the-middle's source) and values, a device tensor [n] or [n, 2] of int32 or int64 indexed like
    the ids the source points into (labels, turn ids, spans, word ids) -> a tensor of source's shape (with a trailing 2 for
    [n, 2]) and values' dtype: values[source] where source >= 0, `fill` (an int: it fills both halves of a pair)
    elsewhere.  One elementwise HIP pass on the current torch stream, never synchronises (it has no scratch); a source at or above
    len(values) gives `fill` and a device-side error that check=True raises as ValueError."""
    if not _is_tensor(source):
        raise TypeError("source must be a torch tensor, not %s" % type(source).__name__)
    if _dtype_name(source) != "int64":
        raise TypeError("source must have dtype int64, not %s" % source.dtype)
    if not source.is_contiguous():
        raise ValueError("source must be contiguous")
    dname, rec = _records_arg("values", values)
    per = 2 if values.dim() == 2 else 1
    if isinstance(fill, bool) or not isinstance(fill, int):
        raise TypeError("fill must be an int, not %s" % type(fill).__name__)
    bits = 31 if dname == "int32" else 63
    if not -2**bits <= fill < 2**bits:
        raise ValueError("fill must fit %s" % dname)
    _on_one_gpu("the gather", (("source", source), ("values", values)))
    import torch
    dev = source.device
    out = torch.empty(tuple(source.shape) + ((2,) if per == 2 else ()), dtype=values.dtype, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.rows_gather_source_device(source.data_ptr(), source.numel(), values.data_ptr(), values.shape[0], rec // per, per,
                                        fill, out.data_ptr(), err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out
    _on_torch_stream(dev, call, used=(source, values, err))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: gather_source: a source at or above the %d values (device-side error %d)"
                         % (values.shape[0], int(err.item())))
    return out


def batch_encode_best_fit(texts, seq_len, *, bos_id=None, eos_id=None, pad_id=0, dtype=None, return_source=False,
                          return_doc_map=False, normalize=None):
    """A list of str: encoded with the initialised context (encode_packed_device), then pack_best_fit.  normalize: as
    batch_encode_padded."""
    _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id), _token_arg("pad_id", pad_id, False)
    _length_arg("seq_len", seq_len, max(1, (bos_id is not None) + (eos_id is not None)))
    _out_width(dtype)
    ids, oo = _texts_to_device(texts, normalize=normalize)
    return pack_best_fit(ids, oo, seq_len, bos_id=bos_id, eos_id=eos_id, pad_id=pad_id, dtype=dtype, check=True,
                         return_source=return_source, return_doc_map=return_doc_map)


def batch_encode_mlm(texts, max_length=None, *, mask_id, seed, vocab_size=None, whole_word=False, mlm_probability=0.15,
                     mask_fraction=0.8, random_fraction=0.1, normalize=None, **collate_kwargs):
    """A list of str -> (input_ids, attention_mask, lengths, labels), a masked-LM training batch: encode_packed_device,
    collate_padded with `collate_kwargs` and its plan, and mask_tokens in place on the rows.  whole_word=True selects
    whole words by token_word_ids_device (the context needs a split preset).  mask_id, seed, vocab_size,
    mlm_probability, mask_fraction, random_fraction: as mask_tokens; normalize: as batch_encode_padded."""
    if not isinstance(whole_word, bool):
        raise TypeError("whole_word must be a bool, not %s" % type(whole_word).__name__)
    if "return_plan" in collate_kwargs:
        raise TypeError("batch_encode_mlm returns no plan: use batch_encode_padded(return_plan=True) and mask_tokens")
    if whole_word and _ctx is not None and _ctx.pretokenizer is None:
        raise ValueError(_NO_PRESET)
    _mlm_args(mask_id, vocab_size, seed, mlm_probability, mask_fraction, random_fraction)
    ids, oo, d_bytes, d_offs = _texts_to_device(texts, with_text=True, normalize=normalize)
    input_ids, mask, lengths, plan = collate_padded(ids, oo, max_length, return_plan=True, **collate_kwargs)
    words = token_word_ids_device(d_bytes, d_offs, ids, oo) if whole_word else None
    _out, labels = mask_tokens(input_ids, plan, mask_id=mask_id, vocab_size=vocab_size, seed=seed,
                               mlm_probability=mlm_probability, mask_fraction=mask_fraction,
                               random_fraction=random_fraction, word_ids=words, inplace=True)
    return input_ids, mask, lengths, labels


# ---- targets: span corruption ---------------------------------------------------------------------------------
_SPAN_LENGTHS = 32  # the lengths a span can be drawn with (SPAN_LEN_MAX of csrc/hutk_collate.hip)


def _span_length_table(mean_span_length, max_span_length, span_length_probs):
    """-> (len_below, tail): len_below[j] = int(P(len <= j + 1) * 2**32), the last entry forced to 2**32;
    tail[j] = P(len > j) for j in 0 .. n_len - 1.  tests/span_ref.py restates this arithmetic."""
    if span_length_probs is not None:
        if isinstance(span_length_probs, (str, bytes)) or not hasattr(span_length_probs, "__len__"):
            raise TypeError("span_length_probs must be a sequence of numbers or None, not %s" % type(span_length_probs).__name__)
        probs = list(span_length_probs)
        if not 1 <= len(probs) <= _SPAN_LENGTHS:
            raise ValueError("span_length_probs must hold 1 .. %d probabilities, not %d" % (_SPAN_LENGTHS, len(probs)))
        for x in probs:
            if isinstance(x, bool) or not isinstance(x, (int, float)):
                raise TypeError("span_length_probs must hold numbers, not %s" % type(x).__name__)
            if not 0 <= x <= 1:  # (NaN is refused too)
                raise ValueError("span_length_probs must hold numbers in [0, 1], not %r" % (x,))
        probs = [float(x) for x in probs]
        if abs(sum(probs) - 1.0) > 1e-9:
            raise ValueError("span_length_probs must sum to 1, not %r" % (sum(probs),))
    else:
        if isinstance(mean_span_length, bool) or not isinstance(mean_span_length, (int, float)):
            raise TypeError("mean_span_length must be a number, not %s" % type(mean_span_length).__name__)
        if not 1 <= mean_span_length < float("inf"):
            raise ValueError("mean_span_length must be at least 1 and finite, not %r" % (mean_span_length,))
        if isinstance(max_span_length, bool) or not isinstance(max_span_length, int):
            raise TypeError("max_span_length must be an int, not %s" % type(max_span_length).__name__)
        if not 1 <= max_span_length <= _SPAN_LENGTHS:
            raise ValueError("max_span_length must be in 1 .. %d, not %d" % (_SPAN_LENGTHS, max_span_length))
        q = 1.0 - 1.0 / float(mean_span_length)  # P(len > j) = q**j in front of the cut
        probs = [(1.0 - q) * q**j for j in range(max_span_length - 1)] + [q**(max_span_length - 1)]
    len_below, tail, cum = [], [], 0.0
    for x in probs:
        tail.append(min(1.0, max(0.0, 1.0 - cum)))
        cum += x
        len_below.append(min(2**32, max(int(cum * 2**32), len_below[-1] if len_below else 0)))
    len_below[-1] = 2**32
    return len_below, tail


def _span_density(p, tail):
    """The asymptotic density of the merged process: a column is noise unless none of the n_len columns at and in
    front of it started a span that reaches it."""
    clear = 1.0
    for t in tail:
        clear *= 1.0 - p * t
    return 1.0 - clear


def _span_start_probability(noise_density, tail):
    """p with _span_density(p, tail) == noise_density, by bisection (the density grows with p).  A density above what
    p = 1 gives raises; with the tails _span_length_table makes (tail[0] == 1) that is a density above 1 only."""
    if noise_density <= 0.0:
        return 0.0
    most = _span_density(1.0, tail)
    if noise_density > most + 1e-12:
        raise ValueError("noise_density %r cannot be reached: spans of these lengths give at most %r" % (noise_density, most))
    if noise_density >= most:
        return 1.0
    lo, hi = 0.0, 1.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if _span_density(mid, tail) < noise_density:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _span_args(dname, sentinel_first, seed, noise_density, mean_span_length, max_span_length, span_length_probs, n_sentinels,
               sentinel_step, target_eos_id, decoder_start_id, max_target_length, pad_id, ignore_index, sides):
    """What corrupt_spans checks of its numbers, before any device call -> (start_below, len_below, eos, start, pad)."""
    bits = 31 if dname == "int32" else 63
    for name, v in (("sentinel_first", sentinel_first), ("n_sentinels", n_sentinels), ("sentinel_step", sentinel_step)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("%s must be an int, not %s" % (name, type(v).__name__))
    _seed_arg(seed)
    if sentinel_step not in (-1, 1):
        raise ValueError("sentinel_step must be -1 or 1, not %d" % sentinel_step)
    if n_sentinels < 0:
        raise ValueError("n_sentinels must not be negative")
    for v in (sentinel_first, sentinel_first + max(n_sentinels - 1, 0) * sentinel_step):
        if not -2**bits <= v < 2**bits:
            raise ValueError("the sentinels %d .. must fit %s: %d does not" % (sentinel_first, dname, v))
    density = _fraction_arg("noise_density", noise_density)
    len_below, tail = _span_length_table(mean_span_length, max_span_length, span_length_probs)
    start_below = int(_span_start_probability(density, tail) * 2**32)
    eos, start = _token_arg("target_eos_id", target_eos_id), _token_arg("decoder_start_id", decoder_start_id)
    pad = _token_arg("pad_id", pad_id, False)
    if max_target_length is not None:
        _length_arg("max_target_length", max_target_length, 1)
    _ignore_arg(ignore_index, dname)
    if sides not in _MLM_SIDES:
        raise ValueError("sides must be 'a', 'b' or 'both', not %r" % (sides,))
    return start_below, len_below, eos, start, pad


def corrupt_spans(input_ids, attention_mask, row_plan, *, sentinel_first, seed, noise_density=0.15, mean_span_length=3.0,
                  max_span_length=10, span_length_probs=None, n_sentinels=100, sentinel_step=-1, target_eos_id=None,
                  decoder_start_id=None, max_target_length=None, pad_id=0, ignore_index=-100, sides="both", check=False):
    """The span corruption (T5-style) of collated rows, one HIP pass: input_ids [n_rows, L] int32 or int64, attention_mask
    uint8 of the same shape and the row_plan of the collate_* call that made them ->
    (input_ids, attention_mask, labels, input_lengths, target_lengths), and decoder_input_ids behind them when
    decoder_start_id is given.  Every noise span of a row becomes ONE sentinel in the corrupted row -- sentinel_first,
    then sentinel_first + sentinel_step and so on (T5 counts down from the top of the vocabulary: step -1) -- and the
    row closes up: whatever side the input was padded on, the output is compact and padded on the right with pad_id,
    with its mask and input_lengths int32 [n_rows].  labels [n_rows, max_target_length] (None: L) holds, for each span in
    order, its sentinel and then its ids, then target_eos_id when given, then ignore_index; what does not fit is
    dropped, and target_lengths int32 [n_rows] is the count before that, so target_lengths > max_target_length tells a
    cut row.  decoder_input_ids is labels moved one column to the right behind decoder_start_id, with pad_id where
    labels holds ignore_index.  Only the columns that hold a token of a text (of side "a", "b" or "both": `sides`) and
    are real by the mask can be noise -- never bos, a separator, eos or padding.  Runs past the n_sentinels-th stay text.
    What is drawn: every eligible column starts a span with probability p, of a length drawn from span_length_probs
    (up to 32 probabilities of the lengths 1, 2, ..; they sum to 1) or, without it, from the geometric law
    P(len > j) = (1 - 1 / mean_span_length)**j cut at max_span_length (at most 32) with the tail folded into the last
    length; a span ends with its side at the latest.  mean_span_length is the mean of that law in front of the cut: the
    drawn lengths have the mean (1 - q**max_span_length) / (1 - q) with q = 1 - 1 / mean_span_length, 2.95 for the
    defaults, and spans that overlap or touch merge, so the runs come out longer than the drawn lengths.  p is found on
    the host by bisection so that a column far from its side's start is noise with probability noise_density,
    1 - prod_j (1 - p * P(len > j)) = noise_density; the few columns at a side's start see fewer predecessors and are
    noise a little less often.  With p = 1 every eligible column starts a span, so every noise_density in [0, 1] can be
    reached with any lengths; only a density outside [0, 1] is refused (ValueError).  The random
    numbers are Philox4x32-10 draws that depend on nothing but (seed, row, column) -- include/hutoken_amd.h states the
    rule in full, tests/span_ref.py restates it in numpy -- so a row's outcome does not depend on the batch around it.
    seed is an int in 0 .. 2**64 - 1 and has no default: there is no hidden state; pass a different one per step.  On the
    current torch stream, never synchronises; check=True does and raises ValueError for a plan that points outside its
    row (nothing is read or written out of bounds either way)."""
    dname, width = _rows_arg("input_ids", input_ids)
    if not _is_tensor(attention_mask):
        raise TypeError("attention_mask must be a torch tensor, not %s" % type(attention_mask).__name__)
    if _dtype_name(attention_mask) != "uint8":
        raise TypeError("attention_mask must have dtype uint8, not %s" % attention_mask.dtype)
    if tuple(attention_mask.shape) != tuple(input_ids.shape) or not attention_mask.is_contiguous():
        raise ValueError("attention_mask must be contiguous and of the shape of input_ids")
    _rows_plan_arg(row_plan, input_ids)
    start_below, len_below, eos, start, pad = _span_args(
        dname, sentinel_first, seed, noise_density, mean_span_length, max_span_length, span_length_probs, n_sentinels,
        sentinel_step, target_eos_id, decoder_start_id, max_target_length, pad_id, ignore_index, sides)
    _on_one_gpu("the corruption", (("input_ids", input_ids), ("attention_mask", attention_mask), ("row_plan", row_plan)))
    import torch
    dev = input_ids.device
    n_rows, L = input_ids.shape
    L_tgt = L if max_target_length is None else max_target_length
    out, out_mask = torch.empty_like(input_ids), torch.empty_like(attention_mask)
    labels = torch.empty((n_rows, L_tgt), dtype=input_ids.dtype, device=dev)
    dec = torch.empty_like(labels) if decoder_start_id is not None else None
    in_lengths, tgt_lengths = (torch.empty(n_rows, dtype=torch.int32, device=dev) for _ in range(2))
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.rows_span_corrupt_device(row_plan.data_ptr(), n_rows, L, input_ids.data_ptr(), width, attention_mask.data_ptr(),
                                       seed, start_below, len_below, sentinel_first, sentinel_step, n_sentinels, eos, start,
                                       pad, ignore_index, _MLM_SIDES[sides], L_tgt, out.data_ptr(), out_mask.data_ptr(),
                                       labels.data_ptr(), 0 if dec is None else dec.data_ptr(), in_lengths.data_ptr(),
                                       tgt_lengths.data_ptr(), err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return (out, out_mask, labels, in_lengths, tgt_lengths) + (() if dec is None else (dec,))
    res = _on_torch_stream(dev, call, used=(input_ids, attention_mask, row_plan, err))
    if check and int(err.item()):
        raise ValueError("hutoken_amd: corrupt_spans: a row_plan that points outside its row (device-side error %d)"
                         % int(err.item()))
    return res


def batch_encode_span_corruption(texts, max_length=None, *, sentinel_first, seed, normalize=None, noise_density=0.15,
                                 mean_span_length=3.0, max_span_length=10, span_length_probs=None, n_sentinels=100,
                                 sentinel_step=-1, target_eos_id=None, decoder_start_id=None, max_target_length=None,
                                 ignore_index=-100, sides="both", check=False, **collate_kwargs):
    """A list of str -> corrupt_spans' (input_ids, attention_mask, labels, input_lengths, target_lengths[,
    decoder_input_ids]), an encoder-decoder training batch: encode_packed_device, collate_padded with `collate_kwargs`
    (its pad_id pads the corrupted rows too) and its plan, then corrupt_spans.  sentinel_first, seed and the
    corruption's keywords: as corrupt_spans (a padded row has an A side only: sides="b" corrupts nothing); check=True is
    handed to both collate_padded and corrupt_spans; normalize: as batch_encode_padded."""
    if "return_plan" in collate_kwargs:
        raise TypeError("batch_encode_span_corruption returns no plan: use batch_encode_padded(return_plan=True) and corrupt_spans")
    pad_id = collate_kwargs.get("pad_id", 0)
    _span_args(_out_width(collate_kwargs.get("dtype"))[1], sentinel_first, seed, noise_density, mean_span_length, max_span_length,
               span_length_probs, n_sentinels, sentinel_step, target_eos_id, decoder_start_id, max_target_length, pad_id,
               ignore_index, sides)
    ids, oo = _texts_to_device(texts, normalize=normalize)
    input_ids, mask, _lengths, plan = collate_padded(ids, oo, max_length, return_plan=True, check=check, **collate_kwargs)
    return corrupt_spans(input_ids, mask, plan, sentinel_first=sentinel_first, seed=seed, noise_density=noise_density,
                         mean_span_length=mean_span_length, max_span_length=max_span_length, span_length_probs=span_length_probs,
                         n_sentinels=n_sentinels, sentinel_step=sentinel_step, target_eos_id=target_eos_id,
                         decoder_start_id=decoder_start_id, max_target_length=max_target_length, pad_id=pad_id,
                         ignore_index=ignore_index, sides=sides, check=check)


# ---- chat: multi-turn conversations --------------------------------------------------------------------------------
_CHATML_ROLES = ("system", "user", "assistant", "tool")
_LLAMA3_ROLES = ("system", "user", "assistant", "ipython")


def _part_arg(what, ids):
    """A prefix or suffix -> tuple of at most 32 int32 values, none of them the C ABI's "absent"."""
    if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple)):
        raise TypeError("%s must be a list or tuple of ints, not %s" % (what, type(ids).__name__))
    ids = tuple(ids)
    if len(ids) > _capi.CHAT_MAX_PART:
        raise ValueError("%s holds %d ids; at most %d" % (what, len(ids), _capi.CHAT_MAX_PART))
    return tuple(_token_arg("an id of %s" % what, v, False) for v in ids)


class ChatTemplate:
    """What surrounds the turns of a conversation (hutk_chat_template, include/hutoken_amd.h): `roles` maps a role's name
    to (prefix_ids, suffix_ids) or (prefix_ids, suffix_ids, n_loss_suffix) -- at most 16 roles, numbered in the dict's
    order, parts of at most 32 ids, n_loss_suffix the number of leading suffix ids that carry loss (default: all) --
    and bos_id / eos_id open and close every conversation (None: absent).  The rendered conversation is
        [bos]  prefix[role] content suffix[role]  (every turn)  [eos, or the prefix of add_generation_prompt's role]
    The table goes to a device when it is first used there (render_chat_device, batch_encode_chat)."""

    def __init__(self, roles, *, bos_id=None, eos_id=None):
        if not isinstance(roles, dict):
            raise TypeError("roles must be a dict {name: (prefix_ids, suffix_ids[, n_loss_suffix])}, not %s" % type(roles).__name__)
        if not 1 <= len(roles) <= _capi.CHAT_MAX_ROLES:
            raise ValueError("a template holds 1 .. %d roles, not %d" % (_capi.CHAT_MAX_ROLES, len(roles)))
        self.role_names, self.parts, self.suffix_loss = [], [], []
        for name, spec in roles.items():
            if not isinstance(name, str):
                raise TypeError("a role's name must be a str, not %s" % type(name).__name__)
            if not isinstance(spec, (list, tuple)) or len(spec) not in (2, 3):
                raise TypeError("role %r must map to (prefix_ids, suffix_ids) or (prefix_ids, suffix_ids, n_loss_suffix)" % (name,))
            pre, suf = _part_arg("the prefix of role %r" % (name,), spec[0]), _part_arg("the suffix of role %r" % (name,), spec[1])
            n_loss = len(suf) if len(spec) == 2 else spec[2]
            if isinstance(n_loss, bool) or not isinstance(n_loss, int):
                raise TypeError("n_loss_suffix of role %r must be an int, not %s" % (name, type(n_loss).__name__))
            if not 0 <= n_loss <= len(suf):
                raise ValueError("n_loss_suffix of role %r must be in 0 .. %d (its suffix), not %d" % (name, len(suf), n_loss))
            self.role_names.append(name)
            self.parts.append((pre, suf))
            self.suffix_loss.append(n_loss)
        self.bos_id, self.eos_id = bos_id, eos_id
        self._bos, self._eos = _token_arg("bos_id", bos_id), _token_arg("eos_id", eos_id)
        self._handles = {}

    def role_index(self, name):
        """The number of role `name`; ValueError for one the template does not hold."""
        if name not in self.role_names:
            raise ValueError("unknown role %r: the template holds %s" % (name, ", ".join(repr(r) for r in self.role_names)))
        return self.role_names.index(name)

    def _handle(self, device_index):
        h = self._handles.get(device_index)
        if h is None:
            h = self._handles[device_index] = _capi.ChatTemplate(self.parts, self.suffix_loss, self._bos, self._eos, device_index)
        return h

    def _loss_mask(self, loss_roles):
        if isinstance(loss_roles, str):
            loss_roles = (loss_roles,)
        if not isinstance(loss_roles, (list, tuple, set, frozenset)):
            raise TypeError("loss_roles must be a sequence of role names, not %s" % type(loss_roles).__name__)
        bits = 0
        for name in loss_roles:
            bits |= 1 << self.role_index(name)
        return bits

    def _gen_role(self, add_generation_prompt):
        if add_generation_prompt is None or add_generation_prompt is False:
            return -1
        if not isinstance(add_generation_prompt, str):
            raise TypeError("add_generation_prompt must be a role's name or None, not %s" % type(add_generation_prompt).__name__)
        r = self.role_index(add_generation_prompt)
        if self.eos_id is not None:
            raise ValueError("a template with an eos_id has no generation prompt: the conversation is closed")
        return r

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}

    @classmethod
    def from_strings(cls, roles, *, bos=None, eos=None):
        """`roles` maps a name to (prefix, suffix) or (prefix, suffix, n_loss_suffix) as STRINGS, encoded with
        encode_special on the initialised context -- the markers must have been installed by set_special_tokens;
        bos / eos: a string that encodes to exactly one id, or None."""
        if not isinstance(roles, dict):
            raise TypeError("roles must be a dict {name: (prefix, suffix[, n_loss_suffix])}, not %s" % type(roles).__name__)
        texts = []
        for name, spec in roles.items():
            if not isinstance(spec, (list, tuple)) or len(spec) not in (2, 3) or not all(isinstance(s, str) for s in spec[:2]):
                raise TypeError("role %r must map to (prefix, suffix) or (prefix, suffix, n_loss_suffix) with two strings" % (name,))
            texts += [spec[0], spec[1]]
        for what, s in (("bos", bos), ("eos", eos)):
            if s is not None and not isinstance(s, str):
                raise TypeError("%s must be a str or None, not %s" % (what, type(s).__name__))
        ends = [(what, s) for what, s in (("bos", bos), ("eos", eos)) if s is not None]
        rows = batch_encode_special(texts + [s for _what, s in ends])
        ids = {}
        for (what, s), row in zip(ends, rows[len(texts):]):
            if len(row) != 1:
                raise ValueError("%s marker %r does not encode to exactly one id (set_special_tokens installs it): %r" % (what, s, row))
            ids[what] = row[0]
        made = {name: (rows[2 * k], rows[2 * k + 1]) + tuple(spec[2:]) for k, (name, spec) in enumerate(roles.items())}
        return cls(made, bos_id=ids.get("bos"), eos_id=ids.get("eos"))

    @staticmethod
    def _markers(markers):
        for m in markers:
            row = encode_special(m)
            if len(row) != 1:
                raise ValueError("marker %r does not encode to exactly one id (set_special_tokens installs it): %r" % (m, row))

    @classmethod
    def chatml(cls, roles=_CHATML_ROLES):
        """ChatML: every turn is <|im_start|>{role}\\n content <|im_end|>\\n, with loss on <|im_end|> but not on the
        newline behind it; no bos, no eos.  Both markers must encode to one id each."""
        cls._markers(("<|im_start|>", "<|im_end|>"))
        return cls.from_strings({r: ("<|im_start|>%s\n" % r, "<|im_end|>\n", 1) for r in roles})

    @classmethod
    def llama3(cls, roles=_LLAMA3_ROLES):
        """Llama 3: <|begin_of_text|>, then every turn is <|start_header_id|>{role}<|end_header_id|>\\n\\n content
        <|eot_id|>; no eos.  The four markers must encode to one id each."""
        cls._markers(("<|begin_of_text|>", "<|start_header_id|>", "<|end_header_id|>", "<|eot_id|>"))
        return cls.from_strings({r: ("<|start_header_id|>%s<|end_header_id|>\n\n" % r, "<|eot_id|>") for r in roles},
                                bos="<|begin_of_text|>")


def render_chat_device(ids, offsets, conv_offsets, roles, template, *, loss_roles=("assistant",), add_generation_prompt=None,
                       ignore_index=-100, n_ids=None, return_turn_ids=False, return_source=False, check=False):
    """The turns of conversations, encoded as one document each (ids int32, offsets int64[n_turns + 1] of an
    encode_*_packed_device call), with roles int32[n_turns] (template.role_index) and conv_offsets int64[n_conv + 1] into
    the turns (from 0 to n_turns), all device tensors -> (out_ids int32[capacity], out_offsets int64[n_conv + 1],
    labels int32[capacity][, turn_ids int32[capacity]][, source int64[capacity]]): one sequence per conversation,
        [bos]  prefix[role] content suffix[role]  (every turn)  tail
    with tail the prefix of role `add_generation_prompt`, or the template's eos.  (out_ids, out_offsets) is a ragged pair
    like the encode's: collate_padded, collate_windows and SequencePacker.add take it unchanged.  labels holds the id on
    the content and the loss-carrying suffix ids of the turns of `loss_roles` and ignore_index elsewhere; turn_ids the
    turn's index inside its conversation (-1 on bos and tail); source the index into `ids` on content tokens (-1
    elsewhere), which carries token_spans_device or token_word_ids_device of the turns over: values[source].  The
    per-token arrays reach rows through gather_rows with the plan of the collate call.  Only the first out_offsets[-1]
    elements are written.  On the current torch stream; synchronises only to read offsets[-1] (not with n_ids=) and for
    check=True, which raises ValueError for a role outside the template, offsets that do not describe ids or
    conv_offsets that do not describe the turns."""
    if not isinstance(template, ChatTemplate):
        raise TypeError("template must be a ChatTemplate, not %s" % type(template).__name__)
    bits = template._loss_mask(loss_roles)
    gen = template._gen_role(add_generation_prompt)
    _ignore_arg(ignore_index, "int32")
    for name, v in (("return_turn_ids", return_turn_ids), ("return_source", return_source)):
        if not isinstance(v, bool):
            raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))

    def sizes():
        if offsets.numel() < 1 or conv_offsets.numel() < 1:
            raise ValueError("offsets and conv_offsets must hold at least one entry")
        if roles.numel() != offsets.numel() - 1:
            raise ValueError("roles must hold one entry per turn (%d), not %d" % (offsets.numel() - 1, roles.numel()))
    _device_tensors((("ids", ids, "int32"), ("offsets", offsets, "int64"), ("conv_offsets", conv_offsets, "int64"),
                     ("roles", roles, "int32")), sizes)
    _on_one_gpu("the render", (("ids", ids), ("offsets", offsets), ("conv_offsets", conv_offsets), ("roles", roles)))
    if n_ids is not None:
        if isinstance(n_ids, bool) or not isinstance(n_ids, int):
            raise TypeError("n_ids must be an int or None")
        if n_ids < 0 or n_ids > ids.numel():
            raise ValueError("n_ids must be in 0 .. ids.numel()")
    import torch
    dev = ids.device
    n_turns, n_conv = offsets.numel() - 1, conv_offsets.numel() - 1
    n_ids = _n_ids(ids, offsets, n_ids)
    h = template._handle(dev.index)
    cap = h.ids_bound(n_conv, n_turns, n_ids, gen)
    turn_offsets = torch.empty(n_turns + 1, dtype=torch.int64, device=dev)
    out_offsets = torch.empty(n_conv + 1, dtype=torch.int64, device=dev)
    out_ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    labels = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    turn_ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_turn_ids else None
    source = torch.empty(max(cap, 1), dtype=torch.int64, device=dev) if return_source else None
    err = torch.zeros(2, dtype=torch.int32, device=dev)  # one word per call
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        h.offsets_device(offsets.data_ptr(), roles.data_ptr(), conv_offsets.data_ptr(), n_conv, n_turns, n_ids, gen,
                         turn_offsets.data_ptr(), out_offsets.data_ptr(), err[0:].data_ptr(), stream)
        h.render_device(ids.data_ptr(), offsets.data_ptr(), roles.data_ptr(), conv_offsets.data_ptr(), turn_offsets.data_ptr(),
                        out_offsets.data_ptr(), n_conv, n_turns, n_ids, gen, bits, ignore_index, cap, out_ids.data_ptr(),
                        labels.data_ptr(), 0 if turn_ids is None else turn_ids.data_ptr(),
                        0 if source is None else source.data_ptr(), err[1:].data_ptr(), stream)
    if check:
        code = int(err.max().item())
        if code:
            raise ValueError("hutoken_amd: render_chat_device: device-side error %d (a role outside the template, offsets that do "
                             "not describe ids, or conv_offsets that do not describe the turns)" % code)
    res = (out_ids, out_offsets, labels)
    if return_turn_ids:
        res += (turn_ids,)
    if return_source:
        res += (source,)
    return res


def _chat_turns(conversations, template):
    """list of conversations -> (contents, role numbers, conv_offsets) as lists; a turn is {"role", "content"} or
    (role, content)."""
    if not isinstance(template, ChatTemplate):
        raise TypeError("template must be a ChatTemplate, not %s" % type(template).__name__)
    if not isinstance(conversations, list):
        raise TypeError("conversations must be a list of conversations (lists of turns), not %s" % type(conversations).__name__)
    contents, roles, conv = [], [], [0]
    for c in conversations:
        if not isinstance(c, (list, tuple)):
            raise TypeError("a conversation must be a list of turns, not %s" % type(c).__name__)
        for turn in c:
            if isinstance(turn, dict):
                if "role" not in turn or "content" not in turn:
                    raise TypeError("a turn must hold 'role' and 'content'")
                role, content = turn["role"], turn["content"]
            elif isinstance(turn, (list, tuple)) and len(turn) == 2:
                role, content = turn
            else:
                raise TypeError("a turn must be a dict {'role', 'content'} or a (role, content) pair, not %s" % type(turn).__name__)
            if not isinstance(content, str):
                raise TypeError("a turn's content must be a str, not %s" % type(content).__name__)
            roles.append(template.role_index(role))
            contents.append(content)
        conv.append(len(contents))
    return contents, roles, conv


def batch_encode_chat(conversations, max_length=None, *, template, loss_roles=("assistant",), add_generation_prompt=None,
                      normalize=None, special=False, byte_fallback=False, truncation="right", padding_side="right", pad_id=0,
                      dtype=None, ignore_index=-100, return_plan=False):
    """A list of conversations -- each a list of {"role", "content"} dicts or (role, content) pairs -> (input_ids
    [n_conv, L], attention_mask, lengths, labels [n_conv, L] of input_ids' dtype[, row_plan]): a supervised fine-tuning
    batch with loss on the turns of `loss_roles` only.  A composition of existing calls on the initialised context's GPU:
    ONE encode call over all contents, render_chat_device with `template`, collate_padded without bos and eos (the render
    wrote them) and its plan, gather_rows of the labels with fill=ignore_index.  The contents are encoded plainly, so
    that a marker's string inside a user's text does NOT become a control id; special=True encodes them with
    encode_special, byte_fallback=True with the byte-fallback table.  add_generation_prompt="assistant" ends every row's
    sequence with that role's prefix (for inference; no loss there).  An unknown role raises ValueError; normalize: as
    batch_encode_padded; max_length, truncation, padding_side, pad_id, dtype: as collate_padded, whose truncation cuts
    the rendered sequence as a whole."""
    contents, roles, conv = _chat_turns(conversations, template)
    template._loss_mask(loss_roles)  # (both raise before anything is encoded)
    template._gen_role(add_generation_prompt)
    _out_width(dtype)
    _ignore_arg(ignore_index, "int32")
    for name, v in (("special", special), ("byte_fallback", byte_fallback)):
        if not isinstance(v, bool):
            raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))
    if byte_fallback:
        ids, oo = _fallback_texts_to_device(contents, special, normalize)
    elif special:
        ids, oo = _special_texts_to_device(contents, normalize)
    else:
        ids, oo = _texts_to_device(contents, normalize=normalize)
    import torch
    dev = ids.device
    d_roles = torch.tensor(roles, dtype=torch.int32, device=dev)
    d_conv = torch.tensor(conv, dtype=torch.int64, device=dev)
    out_ids, out_offsets, labels = render_chat_device(ids, oo, d_conv, d_roles, template, loss_roles=loss_roles,
                                                      add_generation_prompt=add_generation_prompt, ignore_index=ignore_index)
    input_ids, mask, lengths, plan = collate_padded(out_ids, out_offsets, max_length, pad_id=pad_id, truncation=truncation,
                                                    padding_side=padding_side, dtype=dtype, return_plan=True)
    row_labels = gather_rows(plan, input_ids.shape[1], labels, fill=ignore_index).to(input_ids.dtype)
    return (input_ids, mask, lengths, row_labels, plan) if return_plan else (input_ids, mask, lengths, row_labels)


# ---- fill-in-the-middle (csrc/hutk_fim.h, csrc/hutk_collate.hip) ----------------------------------
_FIM_LOSS_BITS = dict({name: 1 << i for i, name in enumerate(_capi.FIM_PARTS)}, end=32)  # HUTK_FIM_PART_*, HUTK_FIM_LOSS_END


def _fim_loss_arg(loss_on):
    """loss_on -> loss_parts of hutk_fim_render_device"""
    if loss_on == "all":
        return 31
    if loss_on == "middle":
        return _FIM_LOSS_BITS["middle"] | _FIM_LOSS_BITS["end"] | _FIM_LOSS_BITS["plain"]
    if isinstance(loss_on, (tuple, list, set, frozenset)) and all(isinstance(x, str) and x in _FIM_LOSS_BITS for x in loss_on):
        bits = 0
        for x in loss_on:
            bits |= _FIM_LOSS_BITS[x]
        return bits
    raise ValueError("loss_on must be 'all', 'middle' or a tuple drawn from ('plain', 'prefix', 'middle', 'suffix', 'sentinel', "
                     "'end'), not %r" % (loss_on,))


def _fim_sentinel_args(prefix_id, suffix_id, middle_id, end_id):
    return (_token_arg("prefix_id", prefix_id, False), _token_arg("suffix_id", suffix_id, False),
            _token_arg("middle_id", middle_id, False), _token_arg("end_id", end_id))


def _fim_draw_args(seed, fim_rate, spm_rate, first_doc):
    """-> (seed, fim_below, spm_below, first_doc): a probability p is the threshold int(p * 2**32) against a draw of 32 bits"""
    _seed_arg(seed)
    fim_below, spm_below = int(_fraction_arg("fim_rate", fim_rate) * 2**32), int(_fraction_arg("spm_rate", spm_rate) * 2**32)
    if isinstance(first_doc, bool) or not isinstance(first_doc, int):
        raise TypeError("first_doc must be an int, not %s" % type(first_doc).__name__)
    if not 0 <= first_doc < 2**62:
        raise ValueError("first_doc must be in 0 .. 2**62 - 1, not %d" % first_doc)
    return seed, fim_below, spm_below, first_doc


def _fim_output_args(ignore_index, return_labels, return_parts, return_source, check):
    _ignore_arg(ignore_index, "int32")
    for name, v in (("return_labels", return_labels), ("return_parts", return_parts), ("return_source", return_source),
                    ("check", check)):
        if not isinstance(v, bool):
            raise TypeError("%s must be a bool, not %s" % (name, type(v).__name__))


def _fim_render(who, ids, n_ids, n_docs, plan_call, used, kinds, sentinels, loss_bits, ignore_index, return_labels,
                return_parts, return_source, check):
    """What fim_device and fim_pieces_device share: the outputs, plan_call(out_offsets, plan, kinds, err, stream) and the
    render behind it on the current torch stream, the check."""
    import torch
    dev = ids.device
    pre, suf, mid, end = sentinels
    cap = _capi.fim_ids_bound(n_docs, n_ids, end != _capi.NO_TOKEN)
    out_offsets = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    plan = torch.empty((max(n_docs, 1), 4), dtype=torch.int64, device=dev)
    if kinds is None:
        kinds = torch.empty(max(n_docs, 1), dtype=torch.int32, device=dev)
    out_ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    labels = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_labels else None
    parts = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_parts else None
    source = torch.empty(max(cap, 1), dtype=torch.int64, device=dev) if return_source else None
    err = torch.zeros(2, dtype=torch.int32, device=dev)  # one word per call
    res = (out_ids, out_offsets) + tuple(t for t in (labels, parts, source) if t is not None)

    def call():
        stream = torch.cuda.current_stream(dev).cuda_stream
        plan_call(out_offsets.data_ptr(), plan.data_ptr(), kinds.data_ptr(), err[0:].data_ptr(), stream)
        _capi.fim_render_device(ids.data_ptr(), plan.data_ptr(), kinds.data_ptr(), out_offsets.data_ptr(), n_docs, n_ids, pre,
                                suf, mid, end, loss_bits, ignore_index, cap, out_ids.data_ptr(),
                                0 if labels is None else labels.data_ptr(), 0 if parts is None else parts.data_ptr(),
                                0 if source is None else source.data_ptr(), err[1:].data_ptr(), stream)
        return res
    _on_torch_stream(dev, call, used=tuple(used) + (ids, plan, kinds, err))
    if check:
        code = int(err.max().item())
        if code:
            raise ValueError("hutoken_amd: %s: device-side error %d (offsets that do not describe ids, or kinds outside 0 .. 2)"
                             % (who, code))
    return res


def fim_device(ids, offsets, *, prefix_id, suffix_id, middle_id, end_id=None, seed, fim_rate=0.5, spm_rate=0.5, first_doc=0,
               loss_on="all", ignore_index=-100, n_ids=None, return_labels=False, return_parts=False, return_source=False,
               check=False):
    """Fill-in-the-middle at token level, on the GPU: the ragged pair of an encode_*_packed_device call (ids int32, offsets
    int64[n_docs + 1]) -> (out_ids int32[capacity], out_offsets int64[n_docs + 1][, labels int32[capacity]][, parts
    int32[capacity]][, source int64[capacity]]).  Document number first_doc + i is transformed with probability fim_rate:
    cut at two places drawn uniformly from its n + 1 gaps into prefix / middle / suffix and written as
        PSM  prefix_id prefix suffix_id suffix middle_id middle [end_id]
        SPM  prefix_id suffix_id suffix middle_id prefix middle [end_id]     (with probability spm_rate)
    and copied unchanged otherwise.  (out_ids, out_offsets) is a ragged pair like the encode's: collate_padded,
    collate_windows and SequencePacker.add take it unchanged, the packer with channels={"labels": labels}.  labels holds
    the id where `loss_on` names the position and ignore_index elsewhere: "all", "middle" (the middle, the end sentinel
    and plain documents) or a tuple drawn from ("plain", "prefix", "middle", "suffix", "sentinel", "end"); parts the
    part of every position (0 plain, 1 prefix, 2 middle, 3 suffix, 4 sentinel); source the index into `ids` on document
    tokens and -1 on sentinels, which carries token_spans_device or token_word_ids_device over: values[source].
    The random numbers are Philox4x32-10 draws that depend on nothing but (seed, first_doc + i) -- include/hutoken_amd.h
    states the rule in full, tests/fim_ref.py restates it in numpy -- so a document's outcome does not depend on the batch
    around it.  seed is an int in 0 .. 2**64 - 1 and has no default: there is no hidden state.  Only the first
    out_offsets[-1] elements are written.  On the current torch stream; synchronises only to read offsets[-1] (not with
    n_ids=) and for check=True, which raises ValueError for offsets that do not describe ids."""
    sentinels = _fim_sentinel_args(prefix_id, suffix_id, middle_id, end_id)
    seed, fim_below, spm_below, first_doc = _fim_draw_args(seed, fim_rate, spm_rate, first_doc)
    bits = _fim_loss_arg(loss_on)
    _fim_output_args(ignore_index, return_labels, return_parts, return_source, check)
    _ragged_args(ids, offsets, n_ids)
    n_docs = offsets.numel() - 1
    n_ids = _n_ids(ids, offsets, n_ids)
    has_end = sentinels[3] != _capi.NO_TOKEN

    def plan_call(d_out_offsets, d_plan, d_kinds, d_err, stream):
        _capi.fim_plan_tokens_device(offsets.data_ptr(), n_docs, n_ids, seed, first_doc, fim_below, spm_below, has_end,
                                     d_out_offsets, d_plan, d_kinds, d_err, stream)
    return _fim_render("fim_device", ids, n_ids, n_docs, plan_call, (offsets,), None, sentinels, bits, ignore_index,
                       return_labels, return_parts, return_source, check)


def fim_cut_text_device(d_bytes, d_offsets, *, seed, fim_rate=0.5, spm_rate=0.5, first_doc=0, check=False):
    """Fill-in-the-middle at character level, first step: the packed text of encode_packed_device (uint8 bytes, int64
    offsets[n_docs + 1], device tensors) -> (piece_offsets int64[3 n_docs + 1], kinds int32[n_docs]).  Every document is
    cut by the draw of fim_device over its BYTES, each cut moved back to the start of its UTF-8 character, into three
    pieces prefix / middle / suffix (a plain document: whole, empty, empty).  No byte is copied: encode the same
    d_bytes with piece_offsets -- ONE encode call over 3 n_docs documents -- and give its (ids, offsets) and `kinds` to
    fim_pieces_device.  No token then straddles a cut.  On the current torch stream, never synchronises; check=True
    does and raises ValueError for offsets that do not describe d_bytes."""
    seed, fim_below, spm_below, first_doc = _fim_draw_args(seed, fim_rate, spm_rate, first_doc)
    if not isinstance(check, bool):
        raise TypeError("check must be a bool, not %s" % type(check).__name__)
    _packed_text_args(d_bytes, d_offsets)
    import torch
    dev = d_bytes.device
    n_docs, n_bytes = d_offsets.numel() - 1, d_bytes.numel()
    pieces = torch.empty(3 * n_docs + 1, dtype=torch.int64, device=dev)
    kinds = torch.empty(max(n_docs, 1), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        _capi.fim_cut_text_device(d_bytes.data_ptr(), d_offsets.data_ptr(), n_docs, n_bytes, seed, first_doc, fim_below,
                                  spm_below, pieces.data_ptr(), kinds.data_ptr(), err.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
        return pieces, kinds
    _on_torch_stream(dev, call, used=(d_bytes, d_offsets, err))
    if check:
        _raise_device_error(err, "fim_cut_text_device")
    return pieces, kinds[:n_docs]


def fim_pieces_device(ids, offsets, kinds, *, prefix_id, suffix_id, middle_id, end_id=None, loss_on="all", ignore_index=-100,
                      n_ids=None, return_labels=False, return_parts=False, return_source=False, check=False):
    """Fill-in-the-middle at character level, second step: (ids int32, offsets int64[3 n_docs + 1]) of ONE encode call over
    the pieces of fim_cut_text_device and its `kinds` int32[n_docs] -> what fim_device returns, with the same keywords
    less the rates and the seed: nothing is drawn here.  Document i is the pieces 3i (prefix), 3i + 1 (middle) and 3i + 2
    (suffix); source indexes `ids`, the pieces' ids."""
    sentinels = _fim_sentinel_args(prefix_id, suffix_id, middle_id, end_id)
    bits = _fim_loss_arg(loss_on)
    _fim_output_args(ignore_index, return_labels, return_parts, return_source, check)

    def sizes():
        if offsets.numel() < 1 or (offsets.numel() - 1) % 3:
            raise ValueError("offsets must hold 3 n_docs + 1 entries, not %d" % offsets.numel())
        if kinds.numel() != (offsets.numel() - 1) // 3:
            raise ValueError("kinds must hold one entry per document (%d), not %d" % ((offsets.numel() - 1) // 3, kinds.numel()))
    _device_tensors((("ids", ids, "int32"), ("offsets", offsets, "int64"), ("kinds", kinds, "int32")), sizes)
    _on_one_gpu("the render", (("ids", ids), ("offsets", offsets), ("kinds", kinds)))
    if n_ids is not None:
        if isinstance(n_ids, bool) or not isinstance(n_ids, int):
            raise TypeError("n_ids must be an int or None")
        if n_ids < 0 or n_ids > ids.numel():
            raise ValueError("n_ids must be in 0 .. ids.numel()")
    n_docs = (offsets.numel() - 1) // 3
    n_ids = _n_ids(ids, offsets, n_ids)
    has_end = sentinels[3] != _capi.NO_TOKEN
    if n_docs == 0:
        import torch
        kinds = torch.zeros(1, dtype=torch.int32, device=ids.device)  # (an empty tensor has no address)

    def plan_call(d_out_offsets, d_plan, d_kinds, d_err, stream):
        _capi.fim_plan_pieces_device(offsets.data_ptr(), d_kinds, n_docs, n_ids, has_end, d_out_offsets, d_plan, d_err, stream)
    return _fim_render("fim_pieces_device", ids, n_ids, n_docs, plan_call, (offsets,), kinds, sentinels, bits, ignore_index,
                       return_labels, return_parts, return_source, check)


def batch_encode_fim(texts, max_length=None, *, prefix_id, suffix_id, middle_id, end_id=None, seed, level="char", fim_rate=0.5,
                     spm_rate=0.5, first_doc=0, loss_on="all", ignore_index=-100, normalize=None, truncation="right",
                     padding_side="right", pad_id=0, dtype=None, return_plan=False):
    """A list of str -> (input_ids [n_docs, L], attention_mask, lengths, labels [n_docs, L] of input_ids' dtype[,
    row_plan]): a fill-in-the-middle pretraining batch.  A composition of existing calls on the initialised context's GPU:
    the upload (and normalize_packed_device), then with level="char" fim_cut_text_device, ONE encode call over the 3
    n_docs pieces and fim_pieces_device -- no token straddles a cut -- or with level="token" one encode call over the
    texts and fim_device; then collate_padded without bos and eos and its plan, and gather_rows of the labels with
    fill=ignore_index.  The sentinels, seed, fim_rate, spm_rate, first_doc and loss_on: as fim_device; max_length,
    truncation, padding_side, pad_id, dtype: as collate_padded, whose truncation cuts the rendered sequence as a whole."""
    sentinels = dict(prefix_id=prefix_id, suffix_id=suffix_id, middle_id=middle_id, end_id=end_id)
    _fim_sentinel_args(**sentinels)
    _fim_draw_args(seed, fim_rate, spm_rate, first_doc)
    _fim_loss_arg(loss_on)
    _ignore_arg(ignore_index, "int32")
    _out_width(dtype)
    if level not in ("char", "token"):
        raise ValueError("level must be 'char' or 'token', not %r" % (level,))
    draw = dict(seed=seed, fim_rate=fim_rate, spm_rate=spm_rate, first_doc=first_doc)
    common = dict(sentinels, loss_on=loss_on, ignore_index=ignore_index, return_labels=True)
    if level == "token":
        ids, oo = _texts_to_device(texts, normalize=normalize)
        out_ids, out_offsets, labels = fim_device(ids, oo, **draw, **common)
    else:
        _normalize_arg(normalize)
        if _ctx is None:
            raise RuntimeError(_NOT_INIT)
        if not isinstance(texts, list):
            raise TypeError("Invalid arguments. Expected a list of strings.")
        import torch
        data, offs = _pack(texts)
        dev = torch.device("cuda", _capi.load().hutk_device_ordinal(_ctx.handle))
        d_bytes = torch.from_numpy(data.copy()).to(dev)  # (a copy: _pack's array is a read-only view of a bytes object)
        d_offs = torch.from_numpy(offs).to(dev)
        with torch.cuda.device(dev):
            if normalize is not None:
                d_bytes, d_offs = normalize_packed_device(d_bytes, d_offs, normalize)
            pieces, kinds = fim_cut_text_device(d_bytes, d_offs, **draw)
            ids, oo = _on_torch_stream(dev, lambda: _encode_device("plain", d_bytes, pieces, 0, True), used=(d_bytes, pieces))
            out_ids, out_offsets, labels = fim_pieces_device(ids, oo, kinds, **common)
    input_ids, mask, lengths, plan = collate_padded(out_ids, out_offsets, max_length, pad_id=pad_id, truncation=truncation,
                                                    padding_side=padding_side, dtype=dtype, return_plan=True)
    row_labels = gather_rows(plan, input_ids.shape[1], labels, fill=ignore_index).to(input_ids.dtype)
    return (input_ids, mask, lengths, row_labels, plan) if return_plan else (input_ids, mask, lengths, row_labels)
