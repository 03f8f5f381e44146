"""The placement yardstick of tests/helpers.py (``placed``, ``guarded_allocations``, ``run_placed``) refuses what it is
there to refuse -- shown on plain Python stand-ins for a kernel, on CPU tensors, the way tests/test_clip_attn.py shows it
for its bounds.  A stand-in gets at memory outside its tensors as a kernel does, by pointer arithmetic
(``as_strided`` past a view's extent, inside the storage the view lies in).  No GPU."""
import numpy as np
import pytest
import torch

import helpers
from helpers import (GUARD_BYTES, INPUT_GUARD, MAX_LEFT_OUT, OUTPUT_GUARD, guarded_allocations, guards_intact, near_crossing, op_cases,
                     placed, poison_left, run_placed)

N = 37


def at(t, k):
    """The one-element view ``&t[0] + k`` -- k may be negative or past the end, as a pointer may."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def in_storage(t, k):
    return 0 <= t.storage_offset() + k < t.untyped_storage().nbytes() // t.element_size()


def poke(t, k, v):
    """A store to ``&t[0] + k``.  Where torch gives the tensor a storage of exactly its size there is nothing to hit, and
    the store is dropped: an ordinary allocation's slack, where nobody sees it."""
    if in_storage(t, k):
        at(t, k)[0] = v


def slack_or_zero(t, k):
    """What a read at ``&t[0] + k`` sees: the storage's content where there is storage, else 0.0 (an ordinary allocation's
    slack: the over-read is harmless there, which is why no test on ordinary allocations notices it)."""
    return float(at(t, k)) if in_storage(t, k) else 0.0


def correct(a, b):
    s, d = torch.empty(N), torch.empty(N)
    torch.add(a, b, out=s)
    torch.sub(a, b, out=d)
    return s, d


def writes_past_the_end(a, b):
    s, d = correct(a, b)
    poke(s, N, 1.0)
    return s, d


def writes_before_the_start(a, b):
    s, d = correct(a, b)
    poke(d, -1, 1.0)
    return s, d


def writes_into_the_other_outputs_guard(a, b):
    s, d = correct(a, b)
    # (computing s, with an index that lands 100 elements behind d)
    poke(d, N + 100, float(s[0]))
    return s, d


def leaves_an_element_unwritten(a, b):
    s, d = torch.empty(N), torch.empty(N)
    torch.add(a[:N - 1], b[:N - 1], out=s[:N - 1])
    torch.sub(a, b, out=d)
    return s, d


def modifies_an_input(a, b):
    s, d = correct(a, b)
    b[3] = 0.0
    return s, d


def reads_past_an_input(a, b):
    s, d = correct(a, b)
    s[N - 1] += 0.0 * slack_or_zero(a, N)              # (even weighted by zero: 0 x NaN is NaN)
    return s, d


def reads_an_index_past_an_input(a, b, idx):
    """(An integer table: what lies outside it is -1, which is no poison -- the comparison with the ordinary run sees it.)"""
    s = torch.empty(N)
    torch.add(a, b, out=s)
    n = torch.empty(1, dtype=torch.int64)
    n[0] = int(idx.sum()) + int(slack_or_zero(idx, idx.numel())) + 1
    return s, n


def inputs():
    g = torch.Generator().manual_seed(3)
    return dict(a=torch.randn(N, generator=g), b=torch.randn(N, generator=g))


@pytest.mark.parametrize("leads", [None, dict(a=4, b=12)])
def test_a_correct_stand_in_passes(leads, monkeypatch):
    got, plain, rec = run_placed(monkeypatch, correct, inputs(), leads=leads, device="cpu")
    assert len(rec.records) == 2 and rec.pass_through_count == 0
    x = inputs()
    assert torch.equal(got[0], x["a"] + x["b"]) and torch.equal(got[1], x["a"] - x["b"])
    assert torch.empty is helpers._raw_empty            # the patches are gone with the call


DEFECTS = [
    (writes_past_the_end, r"written outside a tensor: \(37,\) float32 allocated at test_placement.py:\d+: 4 byte\(s\) changed PAST "
                          r"the end, the nearest 0 byte\(s\) past it"),
    (writes_before_the_start, r"written outside a tensor: \(37,\) float32 allocated at test_placement.py:\d+: 4 byte\(s\) changed "
                              r"BEFORE the start, the nearest 1 byte\(s\) before it"),
    (writes_into_the_other_outputs_guard, r"written outside a tensor: \(37,\) float32 allocated at test_placement.py:\d+: 4 byte\(s\) "
                                          r"changed PAST the end, the nearest 400 byte\(s\) past it"),
    (leaves_an_element_unwritten, r"output 0 \(37,\): 1 element\(s\) hold the allocation's poison: nobody wrote them"),
    (modifies_an_input, r"input b \(37,\) was modified: \d byte\(s\), the first in element 3"),
    (reads_past_an_input, r"output 0 \(37,\): 1 element\(s\) hold the allocation's poison: .* a NaN read outside an input's extent"),
    (reads_an_index_past_an_input, r"output 1 \(placed inputs and guarded allocations vs ordinary ones\): 1 element\(s\) differ, the "
                                   r"first at flat index 0: -1 vs 0"),
]


@pytest.mark.parametrize("stand_in,message", DEFECTS, ids=[d[0].__name__ for d in DEFECTS])
def test_a_defective_stand_in_is_refused_by_name(stand_in, message, monkeypatch):
    if stand_in is reads_an_index_past_an_input:
        with pytest.raises(AssertionError, match=message):
            run_placed(monkeypatch, stand_in, dict(inputs(), idx=torch.tensor([3, -4])), device="cpu")
        return
    with pytest.raises(AssertionError, match=message):
        run_placed(monkeypatch, stand_in, inputs(), device="cpu")
    # ... and on ordinary allocations the same stand-in returns the right numbers: the defect is invisible there
    if stand_in is not leaves_an_element_unwritten:
        x = inputs()
        s, d = stand_in(x["a"].clone(), x["b"].clone())
        assert torch.equal(s, x["a"] + x["b"]) and torch.equal(d, x["a"] - x["b"])


def test_the_guard_that_was_hit_names_its_own_tensor(monkeypatch):
    """A store meant for ``s`` that lands behind ``d`` is reported against ``d``'s allocation (its line), not ``s``'s."""
    with monkeypatch.context() as m:
        rec = guarded_allocations(m, "cpu")
        x = inputs()
        writes_into_the_other_outputs_guard(x["a"], x["b"])
    # (x's tensors came from randn: not one of the four calls, so two records)
    assert [guards_intact(h) for h in rec.records] == [True, False]
    with pytest.raises(AssertionError, match="nearest 400 byte"):
        rec.assert_all_intact()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.int64, torch.int32,
                                   torch.uint8])
@pytest.mark.parametrize("lead_elems", [0, 1, 3])
def test_placed_puts_a_copy_where_it_is_asked_to(dtype, lead_elems):
    t = (torch.arange(11 * 3).reshape(11, 3) % 7).to(torch.float32).to(dtype)
    lead = lead_elems * t.element_size()
    h = placed(t.t(), lead, INPUT_GUARD, "cpu", name="x")            # (a transposed view: the copy is contiguous)
    assert h.t.is_contiguous() and h.t.shape == (3, 11) and h.t.dtype == dtype
    assert torch.equal(h.t.view(torch.uint8), t.t().contiguous().view(torch.uint8))
    assert (h.t.data_ptr() - lead) % 256 == 0
    assert h.lo >= GUARD_BYTES and h.buf.numel() - h.hi >= GUARD_BYTES and h.hi - h.lo == t.numel() * t.element_size()
    assert guards_intact(h) and bool((h.buf[:h.lo] == 0xFF).all()) and bool((h.buf[h.hi:] == 0xFF).all())
    # what an over-read of an input meets: NaN in the floating types, -1 in the integer tables
    outside = torch.as_strided(h.t, (1,), (1,), h.t.storage_offset() + t.numel())
    if dtype.is_floating_point:
        assert bool(torch.isnan(outside.float()).all())
    elif dtype != torch.uint8:
        assert int(outside) == -1
    h.buf[h.hi + GUARD_BYTES - 1] = 0                                  # the last byte of the band still counts
    assert not guards_intact(h)


def test_placed_refuses_a_lead_that_splits_an_element():
    with pytest.raises(AssertionError, match="no multiple of the 4-byte element"):
        placed(torch.zeros(4), 2, INPUT_GUARD, "cpu")


def test_guarded_allocations_place_poison_and_record(monkeypatch):
    raw = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros")}
    with monkeypatch.context() as m:
        rec = guarded_allocations(m, "cpu")
        e = torch.empty((5, 3), dtype=torch.bfloat16)
        el = torch.empty_like(e, dtype=torch.float32)
        z = torch.zeros(7, dtype=torch.int32)
        nz = e.new_zeros((2, 2))
        ws = torch.empty(33, dtype=torch.uint8)
        idx = torch.empty(4, dtype=torch.int64, requires_grad=False)
        gr = torch.empty(3, requires_grad=True)
        cl = torch.empty((2, 6, 4, 5), memory_format=torch.channels_last)
        meta = torch.empty(9, device="meta")
        none = torch.empty(0)
        out = torch.empty(3)
        torch.add(torch.ones(3), 1.0, out=out)
        assert len(rec.records) == 9 and rec.pass_through_count == 0
        assert meta.device.type == "meta" and none.numel() == 0
        for t in (e, el, z, nz, ws, idx, gr, cl, out):
            assert t.data_ptr() % 256 == 0
        assert poison_left(e) == 15 and poison_left(el) == 15 and poison_left(ws) == 33 and poison_left(idx) == 4
        assert poison_left(cl) == cl.numel() and cl.stride() == raw["empty"]((2, 6, 4, 5), memory_format=torch.channels_last).stride()
        assert cl.is_contiguous(memory_format=torch.channels_last)
        assert int(z.abs().sum()) == 0 and float(nz.float().abs().sum()) == 0.0 and nz.dtype == torch.bfloat16
        assert gr.requires_grad and gr.is_leaf and not e.requires_grad
        assert all(bool((h.buf[:h.lo] == OUTPUT_GUARD).all()) and bool((h.buf[h.hi:] == OUTPUT_GUARD).all()) for h in rec.records)
        assert "test_placement.py" in rec.records[0].name
        rec.assert_all_intact()
        # a store anywhere in the storage channels_last spans is inside; one element further is not
        torch.as_strided(cl, (1,), (1,), cl.storage_offset() + cl.numel() - 1)[0] = 1.0
        rec.assert_all_intact()
        torch.as_strided(cl, (1,), (1,), cl.storage_offset() + cl.numel())[0] = 1.0
        with pytest.raises(AssertionError, match=r"\(2, 6, 4, 5\) float32 allocated at test_placement.py"):
            rec.assert_all_intact()
    assert all(getattr(torch, n) is f for n, f in raw.items())


def test_guarded_allocations_leave_other_devices_alone(monkeypatch):
    """Guarding the GPU's allocations (the default) leaves CPU and meta tensors as torch makes them: neither recorded nor
    counted as passed through."""
    with monkeypatch.context() as m:
        rec = guarded_allocations(m)
        a, b = torch.empty(5), torch.zeros(3, device="meta")
        c = a.new_zeros(2)
    assert rec.records == [] and rec.pass_through_count == 0
    assert a._base is None and c._base is None and b.device.type == "meta"


def test_requests_that_come_back_dense_are_placed(monkeypatch):
    """``empty_like`` of a strided slice comes back contiguous and is placed; ``empty_strided`` is not one of the four patched
    calls (nothing in the package calls it) and stays torch's own: neither recorded nor counted."""
    with monkeypatch.context() as m:
        rec = guarded_allocations(m, "cpu")
        t = torch.empty_like(torch.zeros(4, 6)[:, ::2])
        s = torch.empty_strided((3, 3), (8, 1))
        u = torch.empty((3, 3)).t()
    assert len(rec.records) == 3 and rec.pass_through_count == 0          # zeros, empty_like, empty
    assert t.is_contiguous() and t.data_ptr() % 256 == 0 and s.stride() == (8, 1) and s._base is None and u.shape == (3, 3)


def test_an_allocation_that_cannot_be_placed_passes_through_and_is_counted(monkeypatch):
    """A complex tensor (no poison pattern, no kernel of the package takes one) is handed out as torch made it, and the
    recorder says which request that was and where it came from."""
    with monkeypatch.context() as m:
        rec = guarded_allocations(m, "cpu")
        z = torch.empty((2, 3), dtype=torch.complex64)
        e = torch.empty(5)
    assert z._base is None and z.dtype == torch.complex64 and e._base is not None
    assert rec.pass_through_count == 1 and len(rec.records) == 1
    assert rec.passed_through[0].startswith("(2, 3) complex64 allocated at test_placement.py:")


def with_a_complex_scratch(a, b):
    s, d = correct(a, b)
    torch.empty(4, dtype=torch.complex64)
    return s, d


def test_run_placed_refuses_a_pass_through_unless_the_test_lists_it(monkeypatch):
    with pytest.raises(AssertionError, match=r"could not be placed between guards: \['\(4,\) complex64 allocated at test_placement.py:\d+'\]"):
        run_placed(monkeypatch, with_a_complex_scratch, inputs(), device="cpu")
    got, plain, rec = run_placed(monkeypatch, with_a_complex_scratch, inputs(), device="cpu", allowed_pass_through=("(4,) complex64",))
    assert rec.pass_through_count == 1 and len(rec.records) == 2


@pytest.mark.parametrize("case", [c[0] for c in op_cases()])
def test_near_crossing_leaves_out_at_most_one_percent_of_grad_loc(case):
    """tests/test_placement_gpu.py holds grad_loc on these very inputs; the samples ``near_crossing`` takes out of that
    comparison are at most MAX_LEFT_OUT of each case (uniform locations: ~4 * 1e-4 of them lie that close to a crossing)."""
    x = dict(op_cases())[case]
    left_out = near_crossing(x)
    share = float(np.mean(left_out))
    print(f"{case}: {int(left_out[..., 0].sum())} of {left_out[..., 0].size} samples left out ({share:.2%})")
    assert share <= MAX_LEFT_OUT
