"""The chat render without a GPU: the rule's restatement (chat_ref) on rows worked by hand, the Python argument checks,
everything the C ABI refuses before it looks for a device, and hutk_chat_ids_bound against the restatement."""
import ctypes as C
import random

import numpy as np
import pytest

import chat_ref as R
import hutoken_amd as H
from hutoken_amd import _capi

NO = _capi.NO_TOKEN
IGN = -100


def test_names_are_exported():
    for name in ("ChatTemplate", "render_chat_device", "batch_encode_chat"):
        assert name in H.__all__ and hasattr(H, name)
    lib = _capi.load()
    for name in ("hutk_chat_template_create", "hutk_chat_template_destroy", "hutk_chat_ids_bound", "hutk_chat_offsets_device",
                 "hutk_chat_render_device", "hutk_debug_chat_span"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert _capi.chat_span() >= 256 and _capi.chat_span() % 256 == 0


# ---- rows worked by hand ---------------------------------------------------------------------------------------------
def test_worked_conversation_with_bos_and_eos():
    # roles: 0 = user (prefix 10 11, suffix 12), 1 = assistant (prefix 20, suffix 21 22, loss on 21 only)
    tpl = R.Template([[10, 11], [20]], [[12], [21, 22]], suffix_loss=[1, 1], bos=1, eos=2)
    ids = [100, 101, 102, 200, 201, 300]
    offsets = [0, 3, 5, 5, 6]          # user "100 101 102", assistant "200 201", user "", assistant "300"
    roles = [0, 1, 0, 1]
    conv = [0, 2, 2, 4]                # conversation 1 has no turns
    r = R.render(tpl, ids, offsets, roles, conv, loss_roles=0b10)
    assert r["err"] == 0
    assert r["out_ids"].tolist() == [1, 10, 11, 100, 101, 102, 12, 20, 200, 201, 21, 22, 2,
                                     1, 2,
                                     1, 10, 11, 12, 20, 300, 21, 22, 2]
    assert r["labels"].tolist() == [IGN] * 8 + [200, 201, 21, IGN, IGN] + [IGN, IGN] + [IGN] * 5 + [300, 21, IGN, IGN]
    assert r["turn_ids"].tolist() == [-1] + [0] * 6 + [1] * 5 + [-1] + [-1, -1] + [-1] + [0] * 3 + [1] * 4 + [-1]
    assert r["source"].tolist() == [-1, -1, -1, 0, 1, 2, -1, -1, 3, 4, -1, -1, -1] + [-1, -1] + [-1, -1, -1, -1, -1, 5, -1, -1, -1]
    assert r["turn_offsets"].tolist() == [0, 6, 11, 14, 18]
    assert r["out_offsets"].tolist() == [0, 13, 15, 24]
    assert tpl.fixed() == 2 and tpl.bound(3, 4, 6) == 6 + 4 * 3 + 3 * 2


def test_worked_generation_prompt_and_no_bos():
    tpl = R.Template([[10, 11], [20]], [[12], [21, 22]])
    r = R.render(tpl, [100, 200], [0, 1, 2], [0, 1], [0, 1, 2], gen_role=1, loss_roles=0b11)
    assert r["out_ids"].tolist() == [10, 11, 100, 12, 20] + [20, 200, 21, 22, 20]
    assert r["labels"].tolist() == [IGN, IGN, 100, 12, IGN] + [IGN, 200, 21, 22, IGN]
    assert r["turn_ids"].tolist() == [0, 0, 0, 0, -1] + [0, 0, 0, 0, -1]
    assert r["out_offsets"].tolist() == [0, 5, 10] and tpl.fixed(1) == 1 and tpl.fixed(0) == 2 and tpl.fixed() == 0
    # no turns at all: [bos] tail per conversation
    r = R.render(R.Template([[7]], [[]], bos=1), [], [0], [], [0, 0, 0], gen_role=0)
    assert r["out_ids"].tolist() == [1, 7, 1, 7] and r["out_offsets"].tolist() == [0, 2, 4]
    assert r["labels"].tolist() == [IGN] * 4 and r["turn_ids"].tolist() == [-1] * 4


def test_worked_bad_turns_are_left_out():
    tpl = R.Template([[10], [20]], [[12], [21]], eos=2)
    r = R.render(tpl, [100, 101, 102], [0, 1, 2, 3], [0, 99, 1], [0, 3], loss_roles=0b10)
    assert r["err"] == R.E_ARG
    assert r["out_ids"].tolist() == [10, 100, 12, 20, 102, 21, 2]
    assert r["turn_ids"].tolist() == [0, 0, 0, 2, 2, 2, -1]   # the turn keeps its number
    assert r["turn_offsets"].tolist() == [0, 3, 3, 6]
    r = R.render(tpl, [100, 101, 102], [0, 2, 1, 3], [0, 0, 0], [0, 3])  # a negative length in the middle
    assert r["err"] == R.E_ARG and r["out_ids"].tolist() == [10, 100, 101, 12, 10, 101, 102, 12, 2]


# ---- the Python argument checks ----------------------------------------------------------------------------------------
def test_template_argument_checks():
    ok = {"user": ([1, 2], [3]), "assistant": ([4], [5, 6], 1)}
    t = H.ChatTemplate(ok, bos_id=7)
    assert t.role_names == ["user", "assistant"] and t.suffix_loss == [1, 1] and t.role_index("assistant") == 1
    assert t.parts == [((1, 2), (3,)), ((4,), (5, 6))]
    with pytest.raises(ValueError, match="unknown role 'tool'"):
        t.role_index("tool")
    for bad in (None, [("user", ([1], [2]))], "user"):
        with pytest.raises(TypeError, match="roles must be a dict"):
            H.ChatTemplate(bad)
    with pytest.raises(ValueError, match="1 .. 16 roles"):
        H.ChatTemplate({})
    with pytest.raises(ValueError, match="1 .. 16 roles"):
        H.ChatTemplate({"r%d" % i: ([], []) for i in range(17)})
    assert len(H.ChatTemplate({"r%d" % i: ([], []) for i in range(16)}).role_names) == 16
    with pytest.raises(TypeError, match="name must be a str"):
        H.ChatTemplate({1: ([], [])})
    for spec in (([1],), ([1], [2], 1, 1), 5, None):
        with pytest.raises(TypeError, match="must map to"):
            H.ChatTemplate({"user": spec})
    with pytest.raises(TypeError, match="list or tuple of ints"):
        H.ChatTemplate({"user": ("12", [])})
    with pytest.raises(TypeError, match="must be an int"):
        H.ChatTemplate({"user": ([1.5], [])})
    with pytest.raises(TypeError, match="must be an int"):
        H.ChatTemplate({"user": ([True], [])})
    with pytest.raises(ValueError, match="at most 32"):
        H.ChatTemplate({"user": ([], list(range(33)))})
    assert H.ChatTemplate({"user": (list(range(32)), list(range(32)))}).suffix_loss == [32]
    for v in (2**31, -2**31):
        with pytest.raises(ValueError, match="int32"):
            H.ChatTemplate({"user": ([v], [])})
    for n_loss in (-1, 3):
        with pytest.raises(ValueError, match="n_loss_suffix"):
            H.ChatTemplate({"user": ([], [1, 2], n_loss)})
    with pytest.raises(TypeError, match="n_loss_suffix"):
        H.ChatTemplate({"user": ([], [1, 2], 1.0)})
    with pytest.raises(TypeError, match="bos_id"):
        H.ChatTemplate(ok, bos_id="1")
    with pytest.raises(ValueError, match="eos_id"):
        H.ChatTemplate(ok, eos_id=-2**31)
    for bad in (5, None):
        with pytest.raises(TypeError, match="loss_roles"):
            t._loss_mask(bad)
    assert t._loss_mask(()) == 0 and t._loss_mask("assistant") == 2 and t._loss_mask(["user", "assistant"]) == 3
    with pytest.raises(ValueError, match="unknown role"):
        t._loss_mask(("system",))
    assert t._gen_role(None) == -1 and t._gen_role("assistant") == 1
    with pytest.raises(TypeError, match="add_generation_prompt"):
        t._gen_role(1)
    with pytest.raises(ValueError, match="unknown role"):
        t._gen_role("tool")
    with pytest.raises(ValueError, match="no generation prompt"):
        H.ChatTemplate(ok, eos_id=9)._gen_role("assistant")
    with pytest.raises(TypeError, match="two strings"):
        H.ChatTemplate.from_strings({"user": ([1], "x")})
    with pytest.raises(TypeError, match="bos must be a str"):
        H.ChatTemplate.from_strings({"user": ("a", "b")}, bos=5)


def test_render_and_batch_argument_checks():
    import torch
    t = H.ChatTemplate({"user": ([1], [2]), "assistant": ([3], [4])})
    ids = torch.zeros(4, dtype=torch.int32)
    offs = torch.tensor([0, 2, 4], dtype=torch.int64)
    conv = torch.tensor([0, 2], dtype=torch.int64)
    roles = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(TypeError, match="template must be a ChatTemplate"):
        H.render_chat_device(ids, offs, conv, roles, {"user": ([1], [2])})
    with pytest.raises(ValueError, match="unknown role"):
        H.render_chat_device(ids, offs, conv, roles, t, loss_roles=("system",))
    with pytest.raises(ValueError, match="unknown role"):
        H.render_chat_device(ids, offs, conv, roles, t, add_generation_prompt="system")
    with pytest.raises(TypeError, match="ignore_index"):
        H.render_chat_device(ids, offs, conv, roles, t, ignore_index=1.0)
    with pytest.raises(ValueError, match="ignore_index"):
        H.render_chat_device(ids, offs, conv, roles, t, ignore_index=2**31)
    with pytest.raises(TypeError, match="return_source"):
        H.render_chat_device(ids, offs, conv, roles, t, return_source=1)
    with pytest.raises(TypeError, match="roles must be a torch tensor"):
        H.render_chat_device(ids, offs, conv, [0, 1], t)
    with pytest.raises(TypeError, match="roles must have dtype int32"):
        H.render_chat_device(ids, offs, conv, roles.to(torch.int64), t)
    with pytest.raises(TypeError, match="conv_offsets must have dtype int64"):
        H.render_chat_device(ids, offs, conv.to(torch.int32), roles, t)
    with pytest.raises(ValueError, match="one entry per turn"):
        H.render_chat_device(ids, offs, conv, roles[:1], t)
    with pytest.raises(ValueError, match="at least one entry"):
        H.render_chat_device(ids, offs, conv[:0], roles, t)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.render_chat_device(ids, offs, conv, roles, t)
    # the list form: the conversations are checked before anything is encoded (no context is initialised here)
    with pytest.raises(TypeError, match="template must be a ChatTemplate"):
        H.batch_encode_chat([], template=None)
    with pytest.raises(TypeError, match="conversations must be a list"):
        H.batch_encode_chat("hi", template=t)
    with pytest.raises(TypeError, match="a conversation must be a list"):
        H.batch_encode_chat(["hi"], template=t)
    with pytest.raises(TypeError, match="a turn must"):
        H.batch_encode_chat([[("user",)]], template=t)
    with pytest.raises(TypeError, match="a turn must hold"):
        H.batch_encode_chat([[{"role": "user"}]], template=t)
    with pytest.raises(TypeError, match="content must be a str"):
        H.batch_encode_chat([[("user", 5)]], template=t)
    with pytest.raises(ValueError, match="unknown role 'system'"):
        H.batch_encode_chat([[{"role": "system", "content": "x"}]], template=t)
    with pytest.raises(ValueError, match="unknown role"):
        H.batch_encode_chat([[("user", "x")]], template=t, loss_roles=("bot",))
    with pytest.raises(ValueError, match="dtype"):
        H.batch_encode_chat([[("user", "x")]], template=t, dtype="int16")
    with pytest.raises(TypeError, match="special must be a bool"):
        H.batch_encode_chat([[("user", "x")]], template=t, special=1)


# ---- the C ABI: what is refused before a device is looked for ---------------------------------------------------------
def _arr(values):
    return (C.c_int32 * max(1, len(values)))(*values)


def create(n_roles=2, prefix=((1, 2), (3,)), suffix=((4,), (5, 6)), suffix_loss=None, bos=NO, eos=NO, device=-2,
           prefix_offsets=None, suffix_offsets=None, out=True):
    """-> (return code, handle); the parts' offsets are made from the parts unless given."""
    pre = [v for p in prefix for v in p]
    suf = [v for s in suffix for v in s]
    po = list(np.cumsum([0] + [len(p) for p in prefix])) if prefix_offsets is None else prefix_offsets
    so = list(np.cumsum([0] + [len(s) for s in suffix])) if suffix_offsets is None else suffix_offsets
    h = C.c_void_p()
    rc = _capi.load().hutk_chat_template_create(C.byref(h) if out else None, device, n_roles, _arr(pre), _arr(po), _arr(suf),
                                                _arr(so), None if suffix_loss is None else _arr(suffix_loss), bos, eos)
    return rc, h


@pytest.fixture
def host_templates():
    lib = _capi.load()
    made = []

    def make(**kw):
        rc, h = create(**kw)
        assert rc == _capi.OK and h.value
        made.append(h)
        return h
    yield make
    for h in made:
        lib.hutk_chat_template_destroy(h)


def test_template_create_is_checked_before_a_device_is_looked_for():
    import torch
    E = _capi.E_ARG
    assert create(out=False)[0] == E
    for n in (0, -1, 17):
        assert create(n_roles=n)[0] == E
    assert create(prefix=((1,) * 33, (3,)))[0] == E                      # a part longer than 32 ids
    assert create(suffix=((4,), (5,) * 33))[0] == E
    assert create(prefix=((1, NO), (3,)))[0] == E                        # a part holding "absent"
    assert create(suffix=((NO,), (5, 6)))[0] == E
    assert create(prefix_offsets=[1, 2, 3])[0] == E                      # offsets that are not a scan from 0
    assert create(prefix_offsets=[0, 2, 1])[0] == E
    assert create(suffix_offsets=[0, 3, 2])[0] == E
    assert create(suffix_offsets=[0, 40, 41])[0] == E
    for loss in ((2, 0), (0, 3), (-1, 0)):
        assert create(suffix_loss=loss)[0] == E
    assert "suffix_loss" in _capi.last_error()
    lib = _capi.load()
    for loss in (None, (0, 0), (1, 2)):                                  # the same call with good arguments
        rc, h = create(suffix_loss=loss, device=-1)
        assert rc == (_capi.OK if torch.cuda.is_available() else _capi.E_DEVICE)
        lib.hutk_chat_template_destroy(h)
        rc, h = create(suffix_loss=loss)                                   # on the host only: no device is needed
        assert rc == _capi.OK and h.value
        lib.hutk_chat_template_destroy(h)
    rc, h = create(n_roles=16, prefix=((9,) * 32,) * 16, suffix=((8,) * 32,) * 16, bos=1, eos=2)
    assert rc == _capi.OK
    assert lib.hutk_chat_ids_bound(h, 1, 1, 1, -1) == 1 + 64 + 2
    lib.hutk_chat_template_destroy(h)
    lib.hutk_chat_template_destroy(None)


P = 256  # an address that is never read: every check below comes before a device is looked for, and a template on the host only has none


def offsets_call(h, n_conv=2, n_turns=3, n_ids=5, gen=-1, offs=P, roles=P, conv=P, T=P, oo=P, err=None):
    return _capi.load().hutk_chat_offsets_device(h, offs, roles, conv, n_conv, n_turns, n_ids, gen, T, oo, err, None)


def render_call(h, n_conv=2, n_turns=3, n_ids=5, gen=-1, loss=0, cap=64, ids=P, offs=P, roles=P, conv=P, T=P, oo=P, out=P,
                labels=P, turn_ids=None, src=None, err=None):
    return _capi.load().hutk_chat_render_device(h, ids, offs, roles, conv, T, oo, n_conv, n_turns, n_ids, gen, loss, IGN, cap, out,
                                                labels, turn_ids, src, err, None)


def test_device_calls_are_checked_before_a_device_is_looked_for(host_templates):
    E, D = _capi.E_ARG, _capi.E_DEVICE
    h = host_templates()                       # two roles, no bos, no eos
    he = host_templates(eos=9)
    lib = _capi.load()
    # the same calls with good arguments reach the device question
    assert offsets_call(h) == D and render_call(h) == D
    assert offsets_call(h, gen=1) == D and render_call(h, gen=1, loss=3, turn_ids=P, src=P, err=P) == D
    assert offsets_call(he) == D and render_call(he, loss=1) == D
    for call in (offsets_call, render_call):
        assert call(None) == E                                           # no template
        for gen in (-2, 2, 16):
            assert call(h, gen=gen) == E
        assert call(he, gen=0) == E                                      # a generation prompt and an eos
        assert "exclude each other" in _capi.last_error()
        for kw in ({"n_conv": -1}, {"n_turns": -1}, {"n_ids": -1}, {"n_conv": 2**31 - 1}, {"n_turns": 2**31 - 1}):
            assert call(h, **kw) == E
        for name in ("offs", "conv", "T", "oo"):                         # a NULL or misaligned required buffer
            assert call(h, **{name: None}) == E
            assert call(h, **{name: P + 4}) == E
        assert call(h, roles=None) == E and call(h, roles=P + 2) == E
        assert call(h, roles=None, n_turns=0) == D                       # (no turns: no roles are needed)
        assert call(h, err=P + 2) == E
    for loss in (4, 1 << 15, 1 << 31):
        assert render_call(h, loss=loss) == E                            # bits at or above n_roles
    assert render_call(h, cap=-1) == E
    for name in ("ids", "out", "labels"):
        assert render_call(h, **{name: None}) == E
        assert render_call(h, **{name: P + 2}) == E
    assert render_call(h, ids=None, n_ids=0) == D and render_call(h, out=None, labels=None, cap=0) == D
    assert render_call(h, turn_ids=P + 2) == E and render_call(h, src=P + 4) == E
    assert render_call(h, ids=P + 4, out=P + 4, labels=P + 12, turn_ids=P + 8, src=P + 8, offs=P + 8, conv=P + 8, T=P + 8,
                       oo=P + 8) == D                                    # the element's own alignment is enough
    # without conversations there is no work: only out_offsets is needed
    assert offsets_call(h, n_conv=0, n_turns=0, n_ids=0, offs=None, roles=None, conv=None, T=None) == D
    assert offsets_call(h, n_conv=0, n_turns=0, n_ids=0, offs=None, roles=None, conv=None, T=None, oo=None) == E
    assert render_call(h, n_conv=0, n_turns=0, n_ids=0, ids=None, offs=None, roles=None, conv=None, T=None, oo=None,
                       out=None, labels=None) == D
    # the bound: host only
    assert lib.hutk_chat_ids_bound(None, 1, 1, 1, -1) == -E
    for args in ((-1, 1, 1, -1), (1, -1, 1, -1), (1, 1, -1, -1), (1, 1, 1, 2), (1, 1, 1, -2), (2**31 - 1, 1, 1, -1)):
        assert lib.hutk_chat_ids_bound(h, *args) == -E
    assert lib.hutk_chat_ids_bound(he, 1, 1, 1, 0) == -E
    assert lib.hutk_chat_ids_bound(h, 0, 0, 0, -1) == 0
    assert lib.hutk_chat_ids_bound(h, 3, 4, 10, -1) == 10 + 4 * 3 and lib.hutk_chat_ids_bound(h, 3, 4, 10, 0) == 10 + 4 * 3 + 3 * 2
    assert lib.hutk_chat_ids_bound(he, 3, 4, 10, -1) == 10 + 4 * 3 + 3


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.ChatTemplate([((1,), (2,))])
    t = _capi.ChatTemplate([((1,), (2,))], device=-2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        t.offsets_device(P, P, P, 1, 1, 1, -1, P, P)
    with pytest.raises(RuntimeError, match="no HIP device"):
        t.render_device(P, P, P, P, P, P, 1, 1, 1, -1, 0, IGN, 8, P, P)


# ---- the bound ---------------------------------------------------------------------------------------------------------
def random_structure(rng, n_roles, n_conv, max_turns=6, max_len=9, roles=None):
    conv, offsets, role_of = [0], [0], []
    for _ in range(n_conv):
        for _ in range(rng.randrange(max_turns + 1)):
            role_of.append(rng.randrange(n_roles) if roles is None else rng.choice(roles))
            offsets.append(offsets[-1] + rng.randrange(max_len + 1))
        conv.append(len(role_of))
    ids = [rng.randrange(1000, 2000) for _ in range(offsets[-1])]
    return ids, offsets, role_of, conv


def test_ids_bound_holds_and_is_tight(host_templates):
    rng = random.Random(20)
    lib = _capi.load()
    for trial in range(60):
        n_roles = rng.randrange(1, 17)
        prefix = [[rng.randrange(1, 99) for _ in range(rng.randrange(0, 33))] for _ in range(n_roles)]
        suffix = [[rng.randrange(1, 99) for _ in range(rng.randrange(0, 33))] for _ in range(n_roles)]
        bos = rng.choice((None, 5))
        gen = rng.choice((-1, -1, rng.randrange(n_roles)))
        eos = rng.choice((None, 6)) if gen < 0 else None
        tpl = R.Template(prefix, suffix, bos=bos, eos=eos)
        h = host_templates(n_roles=n_roles, prefix=prefix, suffix=suffix, bos=NO if bos is None else bos,
                           eos=NO if eos is None else eos)
        ids, offsets, roles, conv = random_structure(rng, n_roles, rng.randrange(0, 8))
        r = R.render(tpl, ids, offsets, roles, conv, gen_role=gen, loss_roles=rng.randrange(1 << n_roles))
        bound = lib.hutk_chat_ids_bound(h, len(conv) - 1, len(roles), len(ids), gen)
        assert bound == tpl.bound(len(conv) - 1, len(roles), len(ids), gen)
        assert bound >= len(r["out_ids"]) == r["out_offsets"][-1]
        # every turn of a role with the longest prefix + suffix: the bound is the length
        longest = max(range(n_roles), key=lambda q: len(prefix[q]) + len(suffix[q]))
        ids, offsets, roles, conv = random_structure(rng, n_roles, rng.randrange(0, 8), roles=[longest])
        r = R.render(tpl, ids, offsets, roles, conv, gen_role=gen)
        assert lib.hutk_chat_ids_bound(h, len(conv) - 1, len(roles), len(ids), gen) == len(r["out_ids"])
