"""The refusals of ibwa_bsw2_seed_batch's checks and the per-length options (no device needed)."""
import math

import numpy as np
import pytest

from ibwa_amd import engine as E
from tests.test_bsw2_vectors import read_vectors


def _refused(match, seqs, strands, opt="bwasw", adjust=None):
    with pytest.raises(E.IbwaError, match=match):
        E.bsw2_seed_check(seqs, strands, opt, adjust)


def test_check_accepts_valid_input():
    E.bsw2_seed_check([[0, 1, 2, 3]], [0])
    E.bsw2_seed_check([[3], np.zeros(E.BSW2_MAX_LEN, np.uint8)], [1, 0])
    E.bsw2_seed_check([], [])
    E.bsw2_seed_check([[0, 1]], [0], {"is": 0, "t": 1, "bw": 1}, adjust=False)


def test_check_refusals():
    one = [[0, 1, 2]]
    _refused(r"task 1: seq\[2\] = 4 is not below 4", [[0], [0, 1, 4]], [0, 0])
    for key in ("a", "b", "q", "r", "z"):
        _refused(f"{key} 0 < 1", one, [0], {key: 0})
    _refused("is -1 < 0", one, [0], {"is": -1})
    _refused("t 0 < 1", one, [0], {"t": 0}, adjust=False)
    _refused("bw 0 < 1", one, [0], {"bw": 0}, adjust=False)
    E.bsw2_seed_check(one, [0], {"t": 0, "bw": 0}, adjust=True)  # derived from the length then
    _refused("task 0: strand 2", one, [2])
    _refused("task 1: length 0", [[1], []], [0, 0])
    _refused(f"task 0: length {E.BSW2_MAX_LEN + 1} is above {E.BSW2_MAX_LEN}", [np.zeros(E.BSW2_MAX_LEN + 1, np.uint8)], [0])
    assert E.BSW2_MAX_LEN >= 8192


def test_preset_is_bsw2_init_opt():
    o = E.bsw2_opt("bwasw")
    assert (o.a, o.b, o.q, o.r, o.t, o.bw, o.z, o.is_, o.coef, o.adjust) == (1, 3, 5, 2, 30, 50, 1, 3, 5.5, 1)
    with pytest.raises(E.IbwaError, match="nosuch"):
        E.bsw2_opt("nosuch")


def test_opt_for_len_equals_the_vectors():
    seen = set()
    for _name, opt, _strand, _kind, codes, _hits, (t, bw) in read_vectors():
        key = (tuple(sorted(opt.items())), len(codes))
        if key in seen:
            continue
        seen.add(key)
        if opt["adjust"]:
            o = {k: v for k, v in opt.items() if k != "adjust"}
            assert E.bsw2_opt_for_len(o, len(codes)) == (t, bw), (opt, len(codes))
        else:
            assert (opt["t"], opt["bw"]) == (t, bw)
    assert len(seen) > 40


def _trunc(x, y):
    """C's integer division."""
    q = abs(x) // abs(y)
    return q if (x < 0) == (y < 0) else -q


@pytest.mark.parametrize("opt", [dict(a=1, q=5, r=2, t=30, bw=50, coef=5.5), dict(a=2, q=5, r=2, t=60, bw=50, coef=11.0),
                                 dict(a=1, q=2, r=1, t=10, bw=5, coef=5.5), dict(a=1, q=7, r=3, t=37, bw=33, coef=5.5)])
def test_opt_for_len_closed_form(opt):
    """bwtsw2_aux.c:483-497 written out: t = max(t, int(log(l) * coef + .499)) when t < log(l) * coef, then
    bw = min(bw, max(1, min((l a - 2 q) / (2 r + a), (l a - a - t) / r))) with C's division."""
    o = E.bsw2_opt(opt)
    for ln in range(1, 5001):
        t = opt["t"]
        x = math.log(ln) * float(np.float32(opt["coef"]))
        if t < x:
            t = int(x + .499)
        k = min(_trunc(ln * opt["a"] - 2 * opt["q"], 2 * opt["r"] + opt["a"]), _trunc(ln * opt["a"] - opt["a"] - t, opt["r"]))
        want = (t, min(opt["bw"], max(k, 1)))
        assert E.bsw2_opt_for_len(o, ln) == want, ln
