"""The text loss (mmfs_amd/text_loss.py, csrc/mmfs_text_loss.hip), host side: the labels integer for integer against the
reference's fixtures (tests/golden/text_loss_*.npz, made by tests/golden/make_golden_text_loss.py from the reference's
method), the framework route in fp64 against the fixtures' loss and gradient, its reductions and edge cases against the
plain framework statement, the scores of ``generate_scores``, and the C ABI's declarations and argument checks (every one
returns before a launch, so they are safe without a GPU)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden

import mmfs_amd

tl = importlib.import_module("mmfs_amd.text_loss")      # (the package exports the function ``text_loss`` under the module's name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_text_loss_supported", "mmfs_text_loss_forward", "mmfs_text_loss_backward")
CASES = ("plain", "noimage", "offset_int", "offset_list", "offset_tensor", "given")
BAR = 1e-12


def fixture(case):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("text_loss_" + case).items()}
    for k, v in g.items():
        if v.dtype == torch.float32:
            g[k] = v.double()                                   # (stored as fp32 where that is lossless)
    bos, soi, image, pad = (int(x) for x in g["special_ids"])
    g["special"] = dict(bos_token_id=bos, soi_token_id=soi, image_token_id=image, pad_token_id=pad)
    return g


def offset_of(g, case):
    if case == "offset_tensor":
        return g["offset"].long()
    if case == "offset_list":
        return g["offset"].tolist()
    return int(g["offset"])


def labels_of(g, offset, **kw):
    return tl.prepare_gt_text_ids(g["text_ids"], g["attention_mask"], ignore_prompt_token_offset=offset,
                                  ignore_noimage_cond_loss=bool(g["noimage"]), gt_text_ids=g.get("gt_text_ids"),
                                  **g["special"], **kw)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def plain_statement(logits, labels, first=0, **kw):
    """the reference's two lines on rows first .. first + n - 1, in the logits' own precision"""
    n = labels.shape[1]
    return F.cross_entropy(logits.permute(0, 2, 1)[..., first:first + n].contiguous(), labels.contiguous(), **kw)


# ------------------------------------------------------------------ the labels
@pytest.mark.parametrize("case", CASES)
def test_labels_equal_the_fixture(case):
    g = fixture(case)
    got = labels_of(g, offset_of(g, case))
    assert got.dtype == torch.long and got.shape == (4, 23)
    assert torch.equal(got, g["labels"])


def test_the_fixtures_pin_the_quirks():
    """what the golden must hold for the branches to be pinned at all (a guard on the fixture itself)"""
    plain, noimage = fixture("plain"), fixture("noimage")
    ids, bos, soi = plain["text_ids"], plain["special"]["bos_token_id"], plain["special"]["soi_token_id"]
    assert not (ids[1] == bos).any() and (ids[1] == soi).any()                  # a row with no <bos>
    assert ids[2, 0] == bos and ids[2, 1] == soi and plain["labels"][2, 0] == -100      # <bos> -> <soi>
    assert (plain["attention_mask"][3, 11:15] == 0).all() and plain["attention_mask"][3, 15] == 1
    # the first document of row 0 has no image: scored without the flag, ignored with it
    assert (plain["labels"][0, :8] != -100).all() and (noimage["labels"][0, :12] == -100).all()
    # row 1 before its <soi>: nearest_soi = -1 while nearest_bos is clamped to 0
    assert (noimage["labels"][1, :3] == -100).all() and (plain["labels"][1, :3] != -100).all()


def test_the_three_forms_of_the_offset_agree_and_a_wrong_length_raises():
    g = fixture("offset_list")
    offs = g["offset"].tolist()
    want = g["labels"]
    assert torch.equal(labels_of(g, offs), want)
    assert torch.equal(labels_of(g, tuple(offs)), want)
    assert torch.equal(labels_of(g, torch.tensor(offs)), want)
    for k in (0, 3, 30):
        assert torch.equal(labels_of(g, k), labels_of(g, [k] * 4))
        assert torch.equal(labels_of(g, k), labels_of(g, torch.full((4,), k)))
    for bad in ([0, 1, 2], [0] * 5, torch.zeros(3, dtype=torch.long), torch.zeros(4, 1, dtype=torch.long)):
        with pytest.raises(ValueError):
            labels_of(g, bad)


# ------------------------------------------------------------------ the framework route against the fixtures, fp64
@pytest.mark.parametrize("case", CASES)
def test_loss_and_gradient_against_the_fixture(case):
    g = fixture(case)
    x = g["logits"].clone().requires_grad_(True)
    loss = tl.text_loss(x, g["labels"], validate=True)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    assert rel(loss, g["loss"]) <= BAR
    loss.backward()
    assert x.grad.shape == x.shape and rel(x.grad, g["grad.logits"]) <= BAR
    assert float(x.grad[:, -1].abs().max()) == 0.0                              # the last position is never scored


def test_reductions_are_consistent_and_match_the_plain_statement():
    g = fixture("noimage")
    x, labels = g["logits"].float(), g["labels"]
    rows = tl.text_loss(x, labels, reduction="none")
    assert rows.shape == labels.shape and rows.dtype == torch.float32
    assert float(rows[labels == -100].abs().max()) == 0.0
    valid = int((labels != -100).sum())
    total, mean = tl.text_loss(x, labels, reduction="sum"), tl.text_loss(x, labels)
    assert rel(total, rows.double().sum()) <= 1e-6 and rel(mean, rows.double().sum() / valid) <= 1e-6
    for reduction in ("none", "sum", "mean"):
        assert rel(tl.text_loss(x, labels, reduction=reduction), plain_statement(x, labels, reduction=reduction)) <= 1e-6
    # a window: rows 5 .. 12 against 8 labels, and another ignore_index
    sub = labels[:, 5:13].clone()
    sub[sub == -100] = 7
    got = tl.text_loss(x, sub, first=5, ignore_index=7, reduction="none")
    assert rel(got, plain_statement(x, sub, first=5, ignore_index=7, reduction="none")) <= 1e-6
    with pytest.raises(ValueError):
        tl.text_loss(x, labels, first=2)                                         # first + n > L
    with pytest.raises(ValueError):
        tl.text_loss(x, labels.int())
    with pytest.raises(ValueError):
        tl.text_loss(x, labels, reduction="max")


def test_every_label_ignored_is_nan_with_a_zero_gradient_as_the_framework_has_it():
    g = fixture("plain")
    x = g["logits"].float().requires_grad_(True)
    y = g["logits"].float().requires_grad_(True)
    labels = torch.full_like(g["labels"], -100)
    got, want = tl.text_loss(x, labels), plain_statement(y, labels)
    assert torch.isnan(got) and torch.isnan(want)
    got.backward()
    want.backward()
    assert torch.equal(x.grad, torch.zeros_like(x)) and torch.equal(y.grad, torch.zeros_like(y))
    assert float(tl.text_loss(x.detach(), labels, reduction="sum")) == 0.0


@pytest.mark.parametrize("bad", [-1, 40, 1 << 40])
def test_an_out_of_range_label_counts_as_ignored_and_validate_raises(bad):
    g = fixture("plain")
    x, labels = g["logits"].float(), g["labels"].clone()
    where = (labels != -100).nonzero()[3]
    labels[where[0], where[1]] = bad
    with pytest.raises(IndexError):
        tl.text_loss(x, labels, validate=True)
    as_ignored = labels.clone()
    as_ignored[where[0], where[1]] = -100
    for reduction in ("none", "sum", "mean"):
        got = tl.text_loss(x, labels, reduction=reduction)
        assert torch.equal(got, tl.text_loss(x, as_ignored, reduction=reduction, validate=True))
    _, counts = tl._loss_and_counts(x, labels, "mean", -100, 0, None, "test")
    assert counts.dtype == torch.int32 and counts.tolist() == [int((as_ignored != -100).sum()), 1]


def test_option_scores_against_log_softmax_and_gather_on_a_window():
    g = fixture("plain")
    x = g["logits"][:3].float()                                                  # three options over 24 positions
    gen = torch.Generator().manual_seed(3)
    n, context_offset = 6, 9
    ids = torch.randint(0, 40, (3, n), generator=gen)
    mask = torch.ones(3, n, dtype=torch.long)
    mask[1, 4:] = 0
    mask[2, 2:] = 0
    window = x[:, context_offset - 1:context_offset - 1 + n]
    want = (F.log_softmax(window, dim=-1).gather(-1, ids[..., None]).squeeze(-1) * mask).sum(-1)
    got = tl.option_scores(x.requires_grad_(True), ids, mask, context_offset=context_offset)
    assert got.shape == (3,) and not got.requires_grad
    assert rel(got, want) <= 1e-6
    # the reference's own slice ends at -1: the options fill the sequence behind the context
    tail = tl.option_scores(x, ids, mask, context_offset=24 - n)
    want = (F.log_softmax(x[:, 24 - n - 1:-1], dim=-1).gather(-1, ids[..., None]).squeeze(-1) * mask).sum(-1)
    assert rel(tail, want) <= 1e-6


def test_a_forced_kernel_route_on_host_tensors_is_an_error():
    g = fixture("plain")
    with pytest.raises(RuntimeError):
        tl.text_loss(g["logits"].float(), g["labels"], route="kernels")
    with pytest.raises(RuntimeError):
        tl.option_scores(g["logits"].float(), g["labels"].clamp_min(0), torch.ones_like(g["labels"]), context_offset=1,
                         route="kernels")
    with pytest.raises(ValueError):
        tl.text_loss(g["logits"].float(), g["labels"], route="triton")
    assert mmfs_amd.text_loss is tl.text_loss and mmfs_amd.prepare_gt_text_ids is tl.prepare_gt_text_ids
    assert mmfs_amd.option_scores is tl.option_scores


# ------------------------------------------------------------------ the C ABI without a GPU
from helpers import bound_library as _lib  # noqa: E402


def test_new_symbols_are_declared_and_exported_at_abi_14():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n), n
    assert lib.mmfs_msda_abi_version() == 14
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", raw).group(1)) == 14
    assert "mmfs_text_loss_supported" in raw[raw.index("#define MMFS_MSDA_ABI_VERSION"):raw.index("enum mmfs_dtype")]


def test_supported_query_takes_any_row_width():
    f = _lib().mmfs_text_loss_supported
    for dt in (0, 1, 2):
        for V in (1, 2, 7, 9, 513, 32002, 32003, 1 << 24):
            assert f(dt, V) == 1, (dt, V)
        for V in (-3, 0, (1 << 24) + 1):
            assert f(dt, V) == 0, (dt, V)
    assert f(3, 32) == 0 and f(9, 32) == 0 and f(-1, 32) == 0                   # fp64 / unknown dtype


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)                    # never dereferenced on these paths
    DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5

    def fwd(dt=2, B=2, L=8, V=33, first=0, n=7, reduction=2, **named):
        p = dict.fromkeys(("logits", "labels", "loss", "lse", "out", "counts"), fake)
        p.update(named)
        return lib.mmfs_text_loss_forward(dt, *p.values(), B, L, V, first, n, -100, reduction, None)

    def bwd(dt=2, B=2, L=8, V=33, first=0, n=7, reduction=2, **named):
        p = dict.fromkeys(("logits", "labels", "lse", "up", "counts", "grad"), fake)
        p.update(named)
        return lib.mmfs_text_loss_backward(dt, *p.values(), B, L, V, first, n, -100, reduction, None)

    for f in (fwd, bwd):
        assert f(dt=9) == DTYPE and f(dt=3) == DTYPE and f(dt=-1) == DTYPE
        assert f(B=-1) == DIMS and f(L=-1) == DIMS and f(V=-1) == DIMS and f(first=-1) == DIMS and f(n=-1) == DIMS
        assert f(first=2, n=7) == DIMS and f(first=9, n=0) == DIMS                # first + n > L
        assert f(B=1 << 12, L=(1 << 10) + 1, n=3) == DIMS and f(V=(1 << 24) + 1) == DIMS
        assert f(reduction=3) == UNSUPPORTED and f(reduction=-1) == UNSUPPORTED and f(V=0) == UNSUPPORTED
        assert f(logits=None) == NULLPTR and f(labels=None) == NULLPTR and f(lse=None) == NULLPTR
        assert f(logits=ctypes.c_void_p(4104)) == ALIGN and f(labels=odd) == ALIGN and f(lse=ctypes.c_void_p(4098)) == ALIGN
    assert fwd(counts=None) == NULLPTR and fwd(out=None) == NULLPTR and fwd(loss=None) == NULLPTR
    assert bwd(grad=None) == NULLPTR and bwd(up=None) == NULLPTR and bwd(counts=None) == NULLPTR
    assert bwd(counts=None, reduction=1, B=0) == 0 and bwd(B=0, grad=None) == 0     # nothing to write
    assert bwd(grad=ctypes.c_void_p(4104)) == ALIGN
