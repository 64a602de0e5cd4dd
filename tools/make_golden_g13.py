#!/usr/bin/env python3
"""tests/golden/g13_presplit.json: for each split preset, seeded texts over the fixed alphabet of
tests/presplit_cases.py with the match ends (in characters) that the `tokenizers` library gives -- ByteLevel with its
own regex for gpt2, Split(Regex(pattern), "isolated") for cl100k and qwen2.  Needs `tokenizers`; the tests do not.

    python tools/make_golden_g13.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import presplit_cases as PC  # noqa: E402
import importlib  # noqa: E402

PT = importlib.import_module("hutoken_amd.pretokenize")  # (the module: the package's `pretokenize` is a function)


def main():
    import tokenizers
    from tokenizers import Regex, pre_tokenizers
    pts = {
        "gpt2": pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True),
        "cl100k": pre_tokenizers.Split(Regex(PT.PATTERNS["cl100k"]), "isolated"),
        "qwen2": pre_tokenizers.Split(Regex(PT.PATTERNS["qwen2"]), "isolated"),
    }
    out = {"tokenizers_version": tokenizers.__version__, "presets": {}}
    for k, (preset, pt) in enumerate(pts.items()):
        rows = []
        for text in PC.seeded_texts(300, 1300 + k, 10, 150):
            rows.append([text, [span[1] for _piece, span in pt.pre_tokenize_str(text)]])
        out["presets"][preset] = rows
    path = os.path.join(ROOT, "tests", "golden", "g13_presplit.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
        f.write("\n")
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
