"""Which C entry points ``ms_deform_attn_backward`` calls, with which flags and stage bits, for a given (knobs, dtype,
shape, level table): a characterisation of the shim's routing.  The numbers of every route are held to the oracle by
tests/test_op_gpu.py; a route that silently falls through to a slower sequence passes all of that, and fails here.

The expectations, tests/golden/backward_routes.json, were recorded from the shim as it was BEFORE its route decision
became ``_backward_plan`` (``python tests/test_backward_routes_gpu.py --record`` on an MI355X, this file on that tree: it
uses only names both versions have), and are not edited: the shim must go on making the calls it made.
tests/test_backward_routes.py holds ``_backward_plan`` alone, without a device, to the same file.

Each case is one tiny backward, run without the event log (one call per route) and with it (one call per stage)."""
import functools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_routes.json")
PYRAMID = [(16, 16), (8, 8), (4, 4), (2, 2)]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16, "fp64": torch.float64}
KNOBS = {"_taps_algo": "auto", "_taps_prefer_sorted": False, "_bwd_algo": "auto", "_hybrid": True}


def case(dtype="bf16", D=128, Nq=40, H=2, P=4, B=1, levels=PYRAMID, table="registered", lazy=False, value_repeat=None,
         **knobs):
    """``table``: "registered" (canonical, host copy handed over), "fresh" (tensors the shim has never seen) or "gapped"
    (registered, a gap of 3 rows before level 1: not canonical).  ``value_repeat``: a bank of batch 1 serves the B rows."""
    assert set(knobs) <= set(KNOBS)
    return dict(dtype=dtype, D=D, Nq=Nq, H=H, P=P, B=B, levels=levels, table=table, lazy=lazy, value_repeat=value_repeat,
                knobs=knobs)


# The smallest shapes at which the library's host-only answers change: the hybrid workspace needs a 16-bit type, D in
# (32, 64, 128) and Nq >= 32; one LDS-levels kernel serves every level ("taps fused") from Nq >= 64 and Nq*L*P >= 4096 on.
CASES = {
    "1": case(Nq=256),                                      # hybrid, taps fused: no coarse stage
    "2": case(),                                            # hybrid, both taps stages
    "2a": case(_taps_algo="gather"),
    "2b": case(_taps_algo="lds"),                           # the flag makes the taps fused
    "2c": case(lazy=True),
    "2d": case(_hybrid=False),
    "2e": case(_bwd_algo="atomic"),
    "3": case(dtype="fp16", D=32),
    "3lds": case(dtype="fp16", D=32, _taps_algo="lds"),     # the hybrid call refuses, then the library call: raises
    "4": case(dtype="fp32", D=32),                          # no hybrid, no sorted: the library call, or the four staged ones
    "5": case(Nq=16),                                       # 16-bit but Nq < 32: no dense level
    "6": case(table="fresh"),                               # checked on the device: status word passed
    "7": case(table="gapped"),                              # neither levels flag
    "8a": case(dtype="fp32", H=3, D=24, Nq=9, P=3, levels=[(5, 7), (2, 3)]),
    "8b": case(dtype="fp64", D=32, Nq=9, P=2),
    "9a": case(_taps_algo="sorted"),
    "9b": case(dtype="fp32", D=32, _taps_algo="sorted"),    # raises: the route does not apply
    "9c": case(_taps_prefer_sorted=True),
    "9d": case(dtype="fp32", D=32, _taps_prefer_sorted=True),   # silently the library call
    "10": case(levels=[(16, 16), (0, 5), (4, 4)]),          # an empty level in a hybrid call
    "11": case(B=2, value_repeat="tile"),                   # the calls of case 2 at B = 2
}
RUNS = [(name, with_log) for name in CASES for with_log in (False, True)]
run_id = lambda name, with_log: f"{name}/{'log' if with_log else 'nolog'}"

# Position of (flags, stages, workspace pointer, status-word pointer) in the argument list of each backward entry point
# that launches something (include/mmfs_msda.h).  Sizes and addresses are not recorded.
ENTRY_POINTS = {
    "mmfs_msda_backward": dict(ws=10, flags=19),
    "mmfs_msda_backward_checked": dict(ws=10, flags=19, word=20),
    "mmfs_msda_backward_hybrid": dict(ws=12, flags=21, stages=22),
    "mmfs_msda_backward_sorted": dict(ws=10, flags=20, stages=21),
    "mmfs_msda_backward_taps": {},
    "mmfs_msda_backward_value": {},
    "mmfs_msda_backward_value_run": {},
    "mmfs_msda_backward_value_prepare": dict(ws=3),
    "mmfs_msda_backward_value_sort": dict(ws=3),
    "mmfs_msda_backward_value_reduce": dict(ws=3),
}


class RecordingLib:
    """Stands in for ``MSDA._lib``: every attribute is the real library's; calls of the entry points above are noted."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        where = ENTRY_POINTS.get(name)
        if where is None:
            return fn

        def recorded(*args):
            note = {"entry": name}
            for what in ("flags", "stages"):
                if what in where:
                    note[what] = int(args[where[what]])
            for what in ("ws", "word"):
                if what in where:
                    note[what + "_null"] = not args[where[what]]
            self._calls.append(note)
            return fn(*args)
        return recorded


def level_tables(c):
    """(host shapes [L, 2], host start [L], S) of a case, int64 tensors."""
    sh = torch.tensor(c["levels"], dtype=torch.long).reshape(-1, 2)
    px = sh[:, 0] * sh[:, 1]
    st = px.cumsum(0) - px
    S = int(px.sum())
    if c["table"] == "gapped":
        st[1:] += 3
        S += 3
    return sh, st, S


def make_tensors(c, MSDA, dev="cuda"):
    dt = DTYPES[c["dtype"]]
    sh, st, S = level_tables(c)
    B, H, D, Nq, P, L = c["B"], c["H"], c["D"], c["Nq"], c["P"], sh.shape[0]
    g = torch.Generator().manual_seed(7)
    value = torch.rand(1 if c["value_repeat"] else B, S, H, D, generator=g).to(dev, dt)
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g).to(dev, dt)
    attn = torch.rand(B, Nq, H, L, P, generator=g) + 1e-3
    attn = (attn / attn.sum((-1, -2), keepdim=True)).to(dev, dt)
    grad = torch.randn(B, Nq, H * D, generator=g).to(dev, dt)
    dsh, dst = sh.to(dev), st.to(dev)
    if c["table"] != "fresh":
        MSDA.register_level_tables(dsh, dst, S, host_shapes=sh, host_start=st)
    return value, dsh, dst, loc, attn, grad


def observe(mp, name, with_log):
    """Run case ``name`` with ``MSDA._lib`` recording -> (what was observed, the gradients or None, the inputs)."""
    import MultiScaleDeformableAttention as MSDA
    c = CASES[name]
    for knob, v in {**KNOBS, **c["knobs"]}.items():
        mp.setattr(MSDA, knob, v)
    calls, log = [], ([] if with_log else None)
    mp.setattr(MSDA, "_ws_cache", {})
    mp.setattr(MSDA, "_event_log", log)
    mp.setattr(MSDA, "_lib", RecordingLib(MSDA._lib, calls))
    value, sh, st, loc, attn, grad = make_tensors(c, MSDA)
    seen, grads = {}, None
    before = MSDA.route_counts["sorted"]
    try:
        grads = MSDA.ms_deform_attn_backward(value, sh, st, loc, attn, grad, 64, c["lazy"], value_repeat=c["value_repeat"])
        torch.cuda.synchronize()
    except RuntimeError as e:
        seen["raises"] = str(e)
    seen.update(calls=calls, log=[n for n, _, _ in log or []], sorted=MSDA.route_counts["sorted"] - before)
    return seen, grads, (value, loc, attn)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,with_log", RUNS, ids=[run_id(*r) for r in RUNS])
def test_backward_makes_the_recorded_calls(name, with_log, monkeypatch):
    seen, grads, inputs = observe(monkeypatch, name, with_log)
    assert seen == golden()[run_id(name, with_log)]
    if grads is not None:
        for what, g, x in zip(("grad_value", "grad_loc", "grad_attn"), grads, inputs):
            assert g.shape == x.shape and g.dtype == x.dtype, what
            assert bool(torch.isfinite(g).all()), what


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_backward_routes_gpu.py --record"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "mm-interleaved_amd")]
    out = {}
    for run in RUNS:
        with pytest.MonkeyPatch.context() as mp:
            out[run_id(*run)] = observe(mp, *run)[0]
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"recorded {len(out)} runs -> {GOLDEN}")
