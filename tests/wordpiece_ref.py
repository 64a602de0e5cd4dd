"""WordPiece as BERT runs it, restated in plain Python over `unicodedata`: the yardstick of every WordPiece test.

The rule (include/hutoken_amd.h, "WordPiece") is that of the `tokenizers` package:
normalizers.BertNormalizer -> pre_tokenizers.BertPreTokenizer -> models.WordPiece.  Nothing here shares code with
hutoken_amd: the tables of hutoken_amd/wordpiece.py and the kernels are held to this file, and this file to
`tokenizers` where that is installed (test_wordpiece_tokenizers_cpu.py) and to the goldens elsewhere.

A document is a str.  A byte that strict UTF-8 rejects arrives, as everywhere in this project, as the lone surrogate
U+DC80 + (byte - 0x80) of errors="surrogateescape": a character of class "word" that no step changes.
"""
import unicodedata

WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                        + list(range(0x2000, 0x200B)))
assert len(WHITE_SPACE) == 25
# the sixth range starts at U+2B920 as in `tokenizers`, not at U+2B820 as in Google's BERT
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
              (0x2B920, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def is_escape(c):
    return 0xDC80 <= ord(c) <= 0xDCFF


def is_cjk(c):
    o = ord(c)
    return any(a <= o <= b for a, b in CJK_RANGES)


def is_dropped(c):
    """clean_text drops it"""
    if c in "\t\n\r" or is_escape(c):
        return False
    return c in "\x00\ufffd" or unicodedata.category(c) in ("Cc", "Cf", "Co")


def is_space(c):
    return ord(c) in WHITE_SPACE


def is_punct(c):
    o = ord(c)
    if 33 <= o <= 47 or 58 <= o <= 64 or 91 <= o <= 96 or 123 <= o <= 126:
        return True
    return not is_escape(c) and unicodedata.category(c).startswith("P")


def _nfd(s):
    """NFD with the escapes of ill-formed bytes standing still (they are starters no table knows)"""
    out, run = [], []
    for c in s:
        if is_escape(c):
            out.append(unicodedata.normalize("NFD", "".join(run)))
            out.append(c)
            run = []
        else:
            run.append(c)
    out.append(unicodedata.normalize("NFD", "".join(run)))
    return "".join(out)


def normalize(s, lowercase=True, strip_accents=None, clean_text=True, handle_chinese_chars=True):
    if strip_accents is None:
        strip_accents = lowercase
    if clean_text:
        s = "".join(" " if is_space(c) else c for c in s if not is_dropped(c))
    if handle_chinese_chars:
        s = "".join(" %s " % c if is_cjk(c) else c for c in s)
    if strip_accents:
        s = "".join(c for c in _nfd(s) if is_escape(c) or unicodedata.category(c) != "Mn")
    if lowercase:
        s = "".join(c if is_escape(c) else c.lower() for c in s)
    return s


def split(s):
    """the words of a normalised text"""
    words, cur = [], []
    for c in s:
        if is_space(c) or is_punct(c):
            if cur:
                words.append("".join(cur))
                cur = []
            if not is_space(c):
                words.append(c)
        else:
            cur.append(c)
    if cur:
        words.append("".join(cur))
    return words


class Vocab:
    def __init__(self, lines, unk_token="[UNK]", prefix="##", max_input_chars_per_word=100):
        self.ids = {}
        for i, t in enumerate(lines):
            self.ids[t] = i  # (of two equal lines the later id wins)
        self.unk = self.ids[unk_token]
        self.prefix = prefix
        self.max_chars = max_input_chars_per_word

    def match(self, word):
        if len(word) > self.max_chars:
            return [self.unk]
        out, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                piece = word[start:end]
                i = self.ids.get(self.prefix + piece if start else piece)
                if i is not None:
                    break
                end -= 1
            if end == start:
                return [self.unk]
            out.append(i)
            start = end
        return out


def encode(vocab, text, **flags):
    """-> (ids, word_ids) of one document"""
    ids, wids = [], []
    for w, word in enumerate(split(normalize(text, **flags))):
        got = vocab.match(word)
        ids += got
        wids += [w] * len(got)
    return ids, wids


def encode_batch(vocab, texts, **flags):
    """-> (ids, offsets, word_ids): the ragged pair of encode_packed_device and the word ids, as flat lists"""
    ids, offs, wids = [], [0], []
    for t in texts:
        a, b = encode(vocab, t, **flags)
        ids += a
        wids += b
        offs.append(len(ids))
    return ids, offs, wids


def text_of(raw):
    """bytes -> the str the rule is stated on"""
    return raw.decode("utf-8", "surrogateescape")
