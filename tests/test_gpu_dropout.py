"""BPE-dropout on the GPU (csrc/hutk_dropout.hip) against tests/dropout_ref.py, exact in ids and offsets.
Symbols are 32-bit whatever the vocabulary: no case above 65 519 symbols of its own.  Needs an MI355X."""
import random

import numpy as np
import pytest

import dropout_ref as R
import helpers as H
import presplit_ref
from exc_cases import _raw_byte_tokens

pytestmark = pytest.mark.gpu
# name -> (vocabulary seed, dup_ids, merges file, split preset): the built-in splitter, a preset, rank != symbol order, the id-keyed path
CONFIGS = {"plain": (1, False, False, None), "gpt2": (1, False, False, "gpt2"), "dup": (2, True, False, None), "merges": (3, False, True, None)}


@pytest.fixture
def use(tmp_path):
    def use(name):
        """initialize() with the configuration -> (the module, the restatement's model, its split)"""
        import hutoken_amd
        from oracle import oracle
        seed, dup, merges, preset = CONFIGS[name]
        entries, special = H.random_byte_vocab(seed, dup_ids=dup)
        raw = dict(zip(_raw_byte_tokens(entries), (i for _k, i in entries)))
        kw, model = dict(is_byte_encoder=True, pretokenizer=preset), R.StringModel(raw)
        if merges:
            text, ids, rules = H.random_merges_text(entries, 5, noise=False), dict(entries), {}
            kw["merges_file_path"] = H.write_merges(tmp_path, name, text)
            for line in text.splitlines()[1:]:  # (rank: the line's order; the first line is the version comment)
                a, b = (x.encode("utf-8") for x in line.split(" "))
                rules[ids[a], ids[b]] = (len(rules), ids[a + b])
            model = R.RuleModel([raw[bytes([b])] for b in range(256)], rules)
        hutoken_amd.initialize(*H.write_vocab(tmp_path, name, entries, special), device=0, **kw)
        oracle.build()
        return hutoken_amd, model, (lambda doc: presplit_ref.word_starts(doc, preset)) if preset else oracle.split_words
    return use


def _to_device(docs):
    import torch
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    data = np.frombuffer(b"".join(docs) + b"\0" * 16, dtype=np.uint8)[:int(offs[-1])]
    return torch.from_numpy(data.copy()).to("cuda:0"), torch.from_numpy(offs).to("cuda:0")


def _got(pair):
    oo = pair[1].tolist()
    return pair[0][:oo[-1]].tolist(), oo


def _letters(rng, n):
    return bytes(rng.choice(b"qxzetaoinshr") for _ in range(n))


def _texts():
    rng = random.Random(41)
    return [H.random_text(rng, max_words=30).encode("utf-8").replace(b"\0", b"") for _ in range(60)] + [H.merge_loop_words(rng, 200, 2, 40)]


def _edge_docs():
    """a 12-byte word that ends on the first chunk edge and one that crosses the second (the other words are " cd"); one-word
    documents around every tier bound and through the block minima of the long form, a run of one letter among them;
    characters of two to four bytes, empty documents, a document boundary inside a word, 5 000 one-word documents"""
    from hutoken_amd import _capi
    info, rng = _capi.dropout_info(), random.Random(43)
    C, lane, lds = info["chunk_bytes"], info["lane_units"], info["wave_lds_units"]
    fill = b" cd" * ((C - 13) // 3)  # (C - 13 is a multiple of 3 for the chunk of 4096 bytes)
    docs = [b"a" + fill + b" " + _letters(rng, 11) + b" cde" * 2 + fill + b" " + _letters(rng, 11) + b" cd", b""]
    docs += [_letters(rng, n) for n in (lane - 1, lane, lane + 1, 64, 65, lds - 1, lds, lds + 1, 2100, 4097, 20000)] + [b"e" * 3000]
    docs += ["é中 aé中😀a 😀é a😀 文é中文 őű漢".encode(), b"", b"", b"inter", b"national", b" ", b"a"]
    return docs + [_letters(rng, rng.randint(1, 9)) for _ in range(5000)]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_p0_is_the_plain_encoder_and_p1_the_units(use, name):
    hutoken, model, _split = use(name)
    docs = _texts() + _edge_docs()[:21]
    db, do = _to_device(docs)
    assert _got(hutoken.encode_packed_device(db, do, dropout=0.0, seed=1)) == _got(hutoken.encode_packed_device(db, do))
    ids, oo = _got(hutoken.encode_packed_device(db, do, dropout=1.0, seed=1))
    assert oo == do.tolist() and ids == [model.id_of(model.unit(b)) for d in docs for b in d]


@pytest.mark.parametrize("name,p,seed", [("plain", p, seed) for p in (0.1, 0.5, 0.9) for seed in (1, 2**63 + 5)]
                         + [("gpt2", 0.5, 1), ("dup", 0.5, 1), ("merges", 0.5, 1)])
def test_exact_against_the_restatement(use, name, p, seed):
    hutoken, model, split = use(name)
    docs = _edge_docs() + _texts()[:20]
    want = R.encode_docs(model, docs, split, p, seed, first_doc=2**32 - 3)  # (the document number crosses 2^32 inside the batch)
    assert _got(hutoken.encode_packed_device(*_to_device(docs), dropout=p, seed=seed, first_doc=2**32 - 3)) == want


def test_batch_independence_views_and_the_list_forms(use):
    import torch
    hutoken, _model, _split = use("plain")
    docs = _edge_docs()[:40] + _texts()[:10]
    whole = _got(hutoken.encode_packed_device(*_to_device(docs), dropout=0.5, seed=9))
    assert _got(hutoken.encode_packed_device(*_to_device([]), dropout=0.5, seed=9)) == ([], [0])
    for k in (1, 12, len(docs) - 1):  # the documents from k on, numbered from k: the tail of the whole batch
        ids, oo = _got(hutoken.encode_packed_device(*_to_device(docs[k:]), dropout=0.5, seed=9, first_doc=k))
        assert ids == whole[0][whole[1][k]:] and oo == [x - whole[1][k] for x in whole[1][k:]]
    db, do = _to_device(docs)
    view = torch.cat([torch.zeros(3, dtype=torch.uint8, device=db.device), db])[3:]
    assert view.data_ptr() % 16 != 0 and _got(hutoken.encode_packed_device(view, do, dropout=0.5, seed=9)) == whole
    texts = ["inter national", "", "é中 aé中😀a", "qxzq " * 9]
    rows = hutoken.batch_encode_dropout(texts, 0.5, 9, first_doc=4)
    ids, oo = _got(hutoken.encode_packed_device(*_to_device([t.encode() for t in texts]), dropout=0.5, seed=9, first_doc=4))
    assert [t for r in rows for t in r] == ids and [len(r) for r in rows] == np.diff(oo).tolist()
    assert hutoken.encode_dropout(texts[0], 0.5, 9) == hutoken.batch_encode_dropout(texts[:1], 0.5, 9)[0]


def test_a_word_over_262144_bytes_ends_its_document(use):
    import torch
    ctx, (db, do) = use("plain")[0].context(), _to_device([b"ab cd", b"ab " + b"q" * 262145 + b" ab", b"cd ab", b""])
    ids, oo = torch.full((db.numel() + 1,), -7, dtype=torch.int32, device="cuda:0"), torch.full((5,), -7, dtype=torch.int64, device="cuda:0")
    st, err, s = torch.full((4,), -7, dtype=torch.int32, device="cuda:0"), torch.full((1,), -7, dtype=torch.int32, device="cuda:0"), H.side_stream()
    s.wait_stream(torch.cuda.current_stream())
    ctx.encode_dropout_device(db.data_ptr(), do.data_ptr(), 4, db.numel(), 0, 1, 0, ids.data_ptr(), db.numel() + 1, oo.data_ptr(), st.data_ptr(),
                              err.data_ptr(), s.cuda_stream)
    s.synchronize()  # p = 0 against the plain encoder: ids, offsets, status and the note
    plain = H.DeviceBatch(ctx, db.cpu().numpy(), do.cpu().numpy()).run()
    assert (ids[:int(oo[-1])].tolist(), oo.tolist(), st.tolist(), int(err.item())) == tuple(x.tolist() if hasattr(x, "tolist") else x for x in plain)
    assert st.tolist() == [0, 1, 0, 0] and int(err.item()) == H.E_WORD_TOO_LARGE


def test_a_batch_past_2_31_bytes():
    import torch

    import hutoken_amd
    from hutoken_amd import data, synth
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    block, offs = synth.corpus("C3", 4000)
    L = int(offs[-1])
    reps = (2**31 + 2**20) // L + 1
    db = torch.from_numpy(np.ascontiguousarray(block[:L])).to("cuda:0").repeat(reps)
    do = torch.from_numpy(np.concatenate([(offs[:-1][None, :] + L * np.arange(reps, dtype=np.int64)[:, None]).reshape(-1), [L * reps]])).to("cuda:0")
    hashes = []
    for kwargs in (dict(dropout=0.0, seed=1), {}):
        ids, oo = hutoken_amd.encode_packed_device(db, do, **kwargs)
        oo = oo.cpu().numpy()
        hashes.append(H.block_hashes(ids[:int(oo[-1])].cpu().numpy(), oo))
        del ids
    assert db.numel() > 2**31 and hashes[0] == hashes[1] and sum(h["n_ids"] for h in hashes[0]) > 2**27


def test_refusals_on_the_device(tmp_path):
    import torch

    import hutoken_amd
    db, do = _to_device([b"ab cd"])
    entries, special = H.random_char_vocab(1)
    hutoken_amd.initialize(*H.write_vocab(tmp_path, "chars", entries, special), prefix="▁", is_byte_encoder=False, device=0)
    with pytest.raises(ValueError, match="byte-encoder"):
        hutoken_amd.encode_packed_device(db, do, dropout=0.5, seed=1)
    entries, special = H.random_byte_vocab(1)
    hutoken_amd.initialize(*H.write_vocab(tmp_path, "pat", entries, special), is_byte_encoder=True, pattern="[a-z]+", device=0)
    with pytest.raises(ValueError, match="regex pattern"):
        hutoken_amd.encode_packed_device(db, do, dropout=0.5, seed=1)
    ctx, raw = hutoken_amd.context(), (db.data_ptr(), do.data_ptr(), 1, 5)
    out = (torch.zeros(8, dtype=torch.int32, device="cuda:0").data_ptr(), 6, torch.zeros(2, dtype=torch.int64, device="cuda:0").data_ptr())
    for args, exc in (((2**32 + 1, 1, 0), ValueError), ((1, 1, -1), TypeError)):  # (HUTK_E_VALUE; HUTK_E_ARG is TypeError)
        with pytest.raises(exc):
            ctx.encode_dropout_device(*raw, *args, *out)
