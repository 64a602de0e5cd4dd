"""The texts of the row-feature tests (tests/test_features_cpu.py confirms what tests/test_gpu_features.py relies on: the
VG vocabulary encodes them without unknown ids and spans_ref finds every token where its span lies)."""

QUESTIONS = ["Who wrote it?", "", "What is a stride?", "Hol van a kávé?", "How many tokens fit a row of thirty-two?",
             "Mi az árvíztűrő tükörfúrógép?", "Where?", "12345 + 67890 = ?"]
CONTEXTS = ["It was written by nobody in particular.", "An empty question.", " ".join(["A stride is the overlap."] * 20), "",
            "Thirty-two is a small row: we'll see 12345 tokens, they're cut into windows. " * 5,
            "Az árvíztűrő tükörfúrógép egy híres magyar mondat; minden ékezetes betű benne van. " * 4,
            "日本語の龘鬱テキスト 123 és egy kis magyar szöveg\n\nkét sorban, tab\tokkal!!", "1234567890 " * 30]

NER_TEXTS = ["we'll see 12345", "", "Kovács János Budapesten él, a Bartók Béla úton.", " ", "a", "x's", "  \n\n  a",
             "日本語のテキスト 123", "naïve café résumé", "tab\there\tand\n\nthere", "Dr. Szabó-Nagy Éva 2024-ben járt Pécsett!!"]


def short_texts(n=100):
    """n documents shorter than 32 bytes, so that several share one word of the word-start bitmap"""
    words = ["a", " be", " cél", "'s", " 12", "!", "\n", " őz", "é", " x1"]
    return ["".join(words[(i * 7 + k * 3) % len(words)] for k in range(i % 6)) for i in range(n)]


def long_text(n_bytes):
    """one document of at least n_bytes bytes, of words, numbers, contractions and accented letters"""
    piece = "they'll read 1234567 words, árvíztűrő tükörfúrógép és más; "
    return piece * (n_bytes // len(piece.encode("utf-8")) + 1)
