"""Unicode normalisation on the GPU (csrc/hutk_normalize.hip) against tests/norm_ref.py -- the contract itself,
unicodedata.normalize per document -- byte for byte: the text, the offsets and the changed flags, for all four forms.
Needs a real MI355X."""
import numpy as np
import pytest

import norm_ref as R
from view_cases import hungarian as _hungarian

pytestmark = pytest.mark.gpu

FORMS = R.FORMS


def _chunk():
    from hutoken_amd import _capi
    return _capi.norm_chunk_bytes()


def _to_device(docs):
    import torch
    data, offs = R.pack(docs)
    dev = torch.device("cuda", 0)
    return torch.from_numpy(data.copy()).to(dev), torch.from_numpy(offs).to(dev)


def _check(docs, forms=FORMS, **kw):
    """normalize_packed_device(copy=True, return_changed=True) on the batch == the reference, for every form"""
    import hutoken_amd
    db, do = _to_device(docs)
    for form in forms:
        out, oo, ch = hutoken_amd.normalize_packed_device(db, do, form, copy=True, return_changed=True, check=True, **kw)
        rd, ro, rc = R.reference(form, docs)
        assert np.array_equal(oo.cpu().numpy(), ro), form
        assert np.array_equal(ch.cpu().numpy(), rc), form
        got = out.cpu().numpy()
        if not np.array_equal(got, rd):
            bounds = ro.tolist()
            for i in range(len(docs)):
                assert got[bounds[i]:bounds[i + 1]].tobytes() == rd[bounds[i]:bounds[i + 1]].tobytes(), (form, i, docs[i][:64])
        assert out.numel() == len(rd), form


@pytest.mark.parametrize("docs", [[], [b""] * 5, [b"a"], [b"\xcc"], [b""] * 500 + [b"o\xcc\x8b"] + [b""] * 500],
                         ids=["no-docs", "five-empty", "one-byte", "one-bad-byte", "empties-around-dirty"])
def test_empty_and_tiny_batches(docs):
    _check(docs)


@pytest.mark.parametrize("form", FORMS)
def test_all_scalars(form):
    _check(R.scalar_docs(), [form])


def test_named_segments_at_chunk_edges():
    C = _chunk()
    for s, want in zip(R.NAMED, R.NAMED_NFC):
        assert R.norm_doc("NFC", s.encode("utf-8")) == want.encode("utf-8"), s
    _check(R.edge_docs(C))


def test_document_boundaries_inside_segments():
    for batch in R.boundary_batches(_chunk()):
        _check(batch)


def test_long_runs():
    C = _chunk()
    docs = R.long_run_docs(C)
    assert all(len(docs[i]) > 3 * C for i in (1, 3, 5))
    _check(docs)  # the last document is a run that ends at n_bytes


def test_ill_formed_fuzz():
    _check(R.byte_fuzz_docs())
    _check(R.cut_docs(_chunk()))


def test_random_fuzz():
    _check(R.random_docs())


def test_clean_batch_returns_its_input():
    import hutoken_amd
    C = _chunk()
    text = _hungarian(5 * C)
    docs = [p.encode("utf-8") for p in (text[:700], text[700:9000], text[9000:])]
    assert all(R.norm_doc("NFC", d) == d for d in docs)
    db, do = _to_device(docs)
    out, oo, ch = hutoken_amd.normalize_packed_device(db, do, "NFC", return_changed=True)
    assert out is db and oo is do and not ch.any().item()
    out, oo = hutoken_amd.normalize_packed_device(db, do, "NFC", copy=True)
    assert out is not db and oo is not do
    assert out.data_ptr() != db.data_ptr() and bool((out == db).all().item()) and bool((oo == do).all().item())
    docs[-1] += b" szo\xcc\x8blo"  # one decomposed letter in the last document makes it write
    db, do = _to_device(docs)
    out, oo, ch = hutoken_amd.normalize_packed_device(db, do, "NFC", return_changed=True)
    rd, ro, rc = R.reference("NFC", docs)
    assert out is not db and np.array_equal(out.cpu().numpy(), rd) and np.array_equal(oo.cpu().numpy(), ro)
    assert ch.cpu().numpy().tolist() == [0, 0, 1]
    _check(docs)


def test_n_out_path_needs_no_read_and_checks_the_size():
    import hutoken_amd
    docs = R.random_docs()[:3000]
    db, do = _to_device(docs)
    for form in FORMS:
        rd, ro, _rc = R.reference(form, docs)
        out, oo = hutoken_amd.normalize_packed_device(db, do, form, n_out=len(rd))
        assert np.array_equal(out.cpu().numpy(), rd) and np.array_equal(oo.cpu().numpy(), ro)
        out, oo = hutoken_amd.normalize_packed_device(db, do, form, n_out=len(rd), check=True)
        assert np.array_equal(out.cpu().numpy(), rd)
        with pytest.raises(ValueError, match="n_out"):
            hutoken_amd.normalize_packed_device(db, do, form, n_out=len(rd) - 1, check=True)


def test_offsets_that_do_not_describe_the_bytes_raise():
    import torch

    import hutoken_amd
    db, do = _to_device([b"abc", b"de"])
    for bad in ([0, 4, 3], [0, 3, 9], [1, 3, 5]):
        with pytest.raises(ValueError, match="offsets"):
            hutoken_amd.normalize_packed_device(db, torch.tensor(bad, dtype=torch.int64, device=db.device), "NFC")


def test_on_a_side_stream():
    import torch

    import hutoken_amd
    docs = R.random_docs()[:5000] + R.long_run_docs(_chunk())
    db, do = _to_device(docs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(db.device)
    with torch.cuda.stream(side):
        res = [hutoken_amd.normalize_packed_device(db, do, form, copy=True, return_changed=True) for form in FORMS]
    side.synchronize()
    for form, (out, oo, ch) in zip(FORMS, res):
        rd, ro, rc = R.reference(form, docs)
        assert np.array_equal(out.cpu().numpy(), rd) and np.array_equal(oo.cpu().numpy(), ro) and np.array_equal(ch.cpu().numpy(), rc)


def test_host_array_form_and_list_form():
    import importlib

    import hutoken_amd
    from hutoken_amd import _capi
    tables = importlib.import_module("hutoken_amd.normalize")
    docs = R.random_docs()[:2000] + R.byte_fuzz_docs()[:300]
    nz = _capi.Normalizer(tables.table_blob(), 0)
    info = nz.info()
    assert info["chunk_bytes"] == _chunk() and info["lead_bytes"] == [0xCC, 0xC3, 0xC2, 0xC2] and info["max_expansion"] == [3, 3, 11, 11]
    data, offs = R.pack(docs)
    for fi, form in enumerate(FORMS):
        out, oo = nz.batch(fi, data, offs)
        rd, ro, _rc = R.reference(form, docs)
        assert np.array_equal(out, rd) and np.array_equal(oo, ro)
    nz.close()
    texts = [d.decode("utf-8", "surrogateescape") for d in docs]
    import unicodedata
    for form in FORMS:
        assert hutoken_amd.normalize(texts, form) == [unicodedata.normalize(form, t) for t in texts]


@pytest.mark.parametrize("name", ["VL", "VG"])
def test_through_the_encoder(name):
    import unicodedata

    import hutoken_amd
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files(name)
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    pre = ["sz\u0151l\u0151 \u00e9s f\u0171z\u0151", "Gy\u0151r\u00f6tt t\u0171rhet\u0151 az \u0151sz", "\u00c1RV\u00cdZT\u0170R\u0150 t\u00fck\u00f6rf\u00far\u00f3g\u00e9p", "plain ascii text", ""]
    dec = [unicodedata.normalize("NFD", t) for t in pre]
    assert dec[0] != pre[0]
    want = [t.cpu().numpy() for t in hutoken_amd.batch_encode_padded(pre, 32)]
    got = [t.cpu().numpy() for t in hutoken_amd.batch_encode_padded(dec, 32, normalize="NFC")]
    raw = [t.cpu().numpy() for t in hutoken_amd.batch_encode_padded(dec, 32)]
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    assert not np.array_equal(want[0], raw[0])
    try:
        hutoken_amd.set_byte_fallback("auto")
    except ValueError:  # the vocabulary holds no <0xHH> lines: ids of its own for the 256 bytes
        hutoken_amd.set_byte_fallback([1000000 + b for b in range(256)])
    assert hutoken_amd.batch_encode_fallback(dec, normalize="NFC") == hutoken_amd.batch_encode_fallback(pre)
    assert hutoken_amd.batch_encode_fallback(dec) != hutoken_amd.batch_encode_fallback(pre)
    with hutoken_amd.SequencePacker(16, eos_id=1) as a, hutoken_amd.SequencePacker(16, eos_id=1) as b:
        ra, rb = a.add_texts(dec, normalize="NFC"), b.add_texts(pre)
        assert ra["input_ids"].shape[0] > 0
        for k in ra:
            assert np.array_equal(ra[k].cpu().numpy(), rb[k].cpu().numpy()), k
