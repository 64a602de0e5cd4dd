#!/usr/bin/env python3
"""G12 of tests/golden: the compiled reference's answers to tests/test_oracle_vs_reference.py and to the largest word of
tests/test_gpu_parity.py::test_giant_words, so that both run where the reference is not (oracle/_ref, built from the
reference sources by oracle/Makefile).  Run where `make -C oracle ref` has built it.

  calls    per test of test_oracle_vs_reference: every call the test makes of the reference, in order, as
           [method, digest of its arguments, answer] (an answer that raised: {"raised": exception class name});
           each tokenizer's construction as ["init", digest of its arguments with the files' contents, null].
           The tests run here exactly as they are, against the compiled reference, so their assertions hold too.
  giant    the ids of the 262145-byte document of test_giant_words: count and sha256 (int32 little-endian)
"""
import gzip
import hashlib
import json
import locale
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers as H  # noqa: E402
from oracle import oracle, ref  # noqa: E402
import test_oracle_vs_reference as T  # noqa: E402

OUT = H.G12_PATH


class Recorder:
    """ref.RefTokenizer that appends every answer to `log`."""

    def __init__(self, log, *args, **kw):
        log.append(["init", T.init_digest(args, kw), None])
        self.tok, self.log = ref.RefTokenizer(*args, **kw), log

    def _call(self, method, *args):
        entry = [method, T.arg_digest(args)]
        try:
            out = getattr(self.tok, method)(*args)
        except Exception as e:  # noqa: BLE001
            self.log.append(entry + [{"raised": type(e).__name__}])
            raise
        self.log.append(entry + [list(out) if isinstance(out, tuple) else out])
        return out

    def encode(self, text):
        return self._call("encode", text)

    def encode_bytes(self, data):
        return self._call("encode_bytes", data)

    def decode(self, ids):
        return self._call("decode", ids)

    def batch_encode(self, texts, num_threads=1):
        return self._call("batch_encode", texts, num_threads)


def giant():
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    _docs, big = H.giant_word_docs()
    ids, _err = ref.RefTokenizer(vp, sp, kw["prefix"], kw["is_byte_encoder"]).encode_bytes(big)
    return {"n_ids": len(ids), "ids_sha256": hashlib.sha256(np.asarray(ids, dtype="<i4").tobytes()).hexdigest()}


def main():
    assert ref.available(), "build the reference first: make -C oracle ref"
    oracle.build()
    out = {"lc_ctype": locale.setlocale(locale.LC_CTYPE, None), "calls": {}, "giant": giant()}
    for name in sorted(dir(T)):
        if name.startswith("test_"):
            log = out["calls"][name] = []
            getattr(T, name)(pathlib.Path(tempfile.mkdtemp()), oracle, lambda *a, **kw: Recorder(log, *a, **kw))
            print(name, len(log), "calls")
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(out, ensure_ascii=True, separators=(",", ":")).encode())
    print(OUT, os.path.getsize(OUT), "bytes; giant word:", out["giant"]["n_ids"], "ids")


if __name__ == "__main__":
    main()
