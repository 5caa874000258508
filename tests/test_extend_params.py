"""The refusals of ibwa_extend_check and of stdaln_check(mode="extend") (no device): every one names its
pair."""
import numpy as np
import pytest

import ibwa_amd
from ibwa_amd import engine as E


def _refused(match, s1, s2, param, **kw):
    with pytest.raises(E.IbwaError, match=match):
        E.extend_check(s1, s2, param, **kw)


def test_check_accepts_valid_input():
    one = [[0, 1, 2, 3, 4]]
    for mode in ("score", "end", "path"):
        E.extend_check(one, [[4, 3, 2, 1, 0, 0]], "blast", mode=mode)
        E.extend_check(one, one, "bwa", g0=[32000], mode=mode)
        E.extend_check([[], [1]], [[1], []], "blast", mode=mode)
    E.extend_check([[0, 21]], [[20, 3]], "aa2aa", g0=5)
    E.extend_check([], [], "blast")
    # end-cell mode needs no traceback: the longest pair there is
    E.extend_check([np.zeros(1 << 22, np.uint8)], [np.zeros(1 << 22, np.uint8)], "blast", mode="end")
    # path mode: the band bounds the fill, (len2 + band) x len2 cells here
    E.extend_check([np.zeros(1 << 22, np.uint8)], [np.zeros(1000, np.uint8)], "blast", mode="path")
    E.stdaln_check(one, one, "blast", mode="extend")
    E.stdaln_check(one, one, "blast", mode="extend", thres=0)  # the extension has no threshold


def test_parameter_refusals():
    blast = ibwa_amd.aln_param("blast")
    one = [[0, 1, 2]]
    _refused("gap_ext 0", one, one, dict(blast, gap_ext=0))
    _refused("gap_open 0", one, one, dict(blast, gap_open=0))
    _refused("gap_open \\+ gap_ext 701", one, one, dict(blast, gap_open=699))
    _refused("row 1 ", one, one, (5, 2, 2, np.ones(1, np.int32), 1, 50))
    _refused("row 33", one, one, (5, 2, 2, np.ones(33 * 33, np.int32), 33, 50))
    _refused("maximum 0", one, one, dict(blast, matrix=np.minimum(blast["matrix"], 0)))
    _refused("outside -32000..32000", one, one, dict(blast, matrix=blast["matrix"] * 40000))
    with pytest.raises(E.IbwaError, match="mode 3"):
        E._chk(E.lib().ibwa_extend_check(E.c.byref(E._aln_param_struct("blast")[0]), 3, 0, None, None, None, None, None, None, None))
    with pytest.raises(KeyError):
        E.extend_check(one, one, blast, mode="local")


def test_pair_refusals_name_the_pair():
    blast = ibwa_amd.aln_param("blast")
    one, two = [[0, 1, 2]], [[0, 1, 2], [3, 2, 1]]
    _refused("pair 0: G0 0 outside 1..32000", one, one, blast, g0=0)
    _refused("pair 1: G0 32001 outside 1..32000", two, two, blast, g0=[1, 32001])
    _refused("pair 1: G0 -4", two, two, blast, g0=[7, -4])
    _refused(r"pair 0: seq1\[1\] = 5 is not below row 5", [[0, 5, 1]], one, blast)
    _refused(r"pair 1: seq2\[0\] = 9 is not below row 5", [[0], [1]], [[1], [9]], blast)
    _refused(r"pair 0: length 4194305 / 3 is past", [np.zeros((1 << 22) + 1, np.uint8)], one, blast)
    _refused(r"pair 1: length 1 / 4194305 is past", [[0], [1]], [[0], np.zeros((1 << 22) + 1, np.uint8)], blast)
    # path mode: (w1 + 1) x (w2 + 1) cells with w1 = min(len1, len2 + band - 1), w2 = min(len2, len1 + band)
    big = np.zeros(6000, np.uint8)
    _refused(r"pair 1: the path fill of 6000 x 6000 in band 12000 can take \(6000 \+ 1\) x \(6000 \+ 1\) cells", [[0], big],
             [[0], big], dict(blast, band_width=0), mode="path")
    E.extend_check([big], [big], dict(blast, band_width=0), mode="end")
    E.extend_check([big], [big], dict(blast, band_width=0), mode="score")
    E.extend_check([big[:5000]], [big[:5000]], dict(blast, band_width=0), mode="path")
    # scores as large as the matrix allows next to the global core's -2^30
    huge = dict(blast, matrix=np.where(np.eye(5, dtype=bool), 32000, -32000).astype(np.int32))
    # 33 000 + 900 symbols (29.7 M cells, inside the traceback bound) x 32 000 per cell >= 2^30
    wide, flat = np.zeros(33000, np.uint8), np.zeros(900, np.uint8)
    _refused(r"pair 0: \(33000 \+ 900\) symbols x 32000 per cell can pass 2\^30", [wide], [flat], dict(huge, band_width=0), mode="path")
    E.extend_check([wide], [flat], dict(huge, band_width=0), mode="end")
    E.extend_check([wide], [flat], dict(blast, band_width=0), mode="path")


def test_stdaln_check_extend_refusals():
    blast = ibwa_amd.aln_param("blast")
    big = np.zeros(6000, np.uint8)
    with pytest.raises(E.IbwaError, match=r"pair 0: the path fill of 6000 x 6000"):
        E.stdaln_check([big], [big], dict(blast, band_width=0), mode="extend")
    with pytest.raises(E.IbwaError, match=r"pair 0: seq1\[0\] = 6 is not below row 5"):
        E.stdaln_check([[6]], [[1]], blast, mode="extend")
    with pytest.raises(E.IbwaError, match="gap_ext 0"):
        E.stdaln_check([[1]], [[1]], dict(blast, gap_ext=0), mode="extend")
    with pytest.raises(E.IbwaError, match="type 3 is none of"):
        E._chk(E.lib().ibwa_stdaln_check(E.c.byref(E._aln_param_struct("blast")[0]), 3, 1, 0, None, None, None, None, None, None))
