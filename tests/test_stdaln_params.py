"""The alignment presets and the refusals of ibwa_stdaln_batch's checks (no device needed).

The presets (ibwa_aln_param_preset) are compared value for value with the reference's own
aln_param_blast / aln_param_aa2aa / aln_param_bwa, read through ctypes from the compiled reference
(oracle/_ref/libibwa_ref.so); the refusals go through ibwa_stdaln_check, the checks that
ibwa_stdaln_batch runs before it touches the device.
"""
import ctypes
import os

import numpy as np
import pytest

import ibwa_amd
import oracle
from ibwa_amd import engine as E


class RefAlnParam(ctypes.Structure):
    _fields_ = [("gap_open", ctypes.c_int), ("gap_ext", ctypes.c_int), ("gap_end", ctypes.c_int),
                ("matrix", ctypes.POINTER(ctypes.c_int)), ("row", ctypes.c_int), ("band_width", ctypes.c_int)]


@pytest.mark.skipif(not os.path.exists(oracle.REF_LIB), reason="the compiled reference is not here")
@pytest.mark.parametrize("name", ["blast", "aa2aa", "bwa"])
def test_preset_equals_reference(name):
    L = ctypes.CDLL(oracle.REF_LIB, mode=os.RTLD_LAZY)
    ref = RefAlnParam.in_dll(L, "aln_param_" + name)
    got = ibwa_amd.aln_param(name)
    assert (got["gap_open"], got["gap_ext"], got["gap_end"], got["row"], got["band_width"]) == \
        (ref.gap_open, ref.gap_ext, ref.gap_end, ref.row, ref.band_width)
    want = np.array([ref.matrix[k] for k in range(ref.row * ref.row)], np.int32).reshape(ref.row, ref.row)
    assert got["matrix"].shape == want.shape
    assert (got["matrix"] == want).all(), np.argwhere(got["matrix"] != want)[:5]
    if name == "aa2aa":
        sm = (ctypes.c_int * (22 * 22)).in_dll(L, "aln_sm_blosum62")
        assert got["matrix"].ravel().tolist() == list(sm)


def test_presets_without_reference():
    """What the issue states about the presets, whether or not the reference is at hand."""
    b = ibwa_amd.aln_param("blast")
    assert (b["gap_open"], b["gap_ext"], b["gap_end"], b["row"], b["band_width"]) == (5, 2, 2, 5, 50)
    m = b["matrix"]
    assert all(m[x, y] == (-2 if 4 in (x, y) else 1 if x == y else -3) for x in range(5) for y in range(5))
    a = ibwa_amd.aln_param("aa2aa")
    assert (a["gap_open"], a["gap_ext"], a["gap_end"], a["row"], a["band_width"]) == (10, 2, 2, 22, 50)
    m = a["matrix"]
    order = "ARNDCQEGHILKMFPSTWYV*X"
    assert (m == m.T).all()
    assert [int(m[k, k]) for k in range(22)] == [4, 5, 6, 6, 9, 5, 5, 6, 8, 4, 4, 5, 5, 6, 7, 4, 5, 11, 7, 4, 1, -1]
    assert m[order.index("W"), order.index("F")] == 1 and m[order.index("*"), order.index("A")] == -4
    with pytest.raises(E.IbwaError, match="nosuch"):
        ibwa_amd.aln_param("nosuch")


def _refused(match, s1, s2, param, **kw):
    with pytest.raises(E.IbwaError, match=match):
        E.stdaln_check(s1, s2, param, **kw)


def test_check_accepts_valid_input():
    E.stdaln_check([[0, 1, 2, 3, 4]], [[4, 3, 2, 1, 0, 0]], "blast")
    E.stdaln_check([[0, 21]], [[20, 3]], "aa2aa", mode="global")
    E.stdaln_check([np.zeros(1024, np.uint8)], [np.zeros(16384, np.uint8)], "aa2aa", mode="global")
    E.stdaln_check([np.zeros(1024, np.uint8)], [np.zeros(1 << 22, np.uint8)], "aa2aa")


def test_check_refusals():
    blast = ibwa_amd.aln_param("blast")
    one = [[0, 1, 2]]
    _refused("gap_ext 0", one, one, dict(blast, gap_ext=0))
    _refused("gap_open 0", one, one, dict(blast, gap_open=0))
    _refused("row 1 ", one, one, (5, 2, 2, np.ones(1, np.int32), 1, 50))
    _refused("row 33", one, one, (5, 2, 2, np.ones(33 * 33, np.int32), 33, 50))
    _refused("maximum 0", one, one, dict(blast, matrix=np.minimum(blast["matrix"], 0)))
    _refused(r"seq1\[1\] = 5 is not below row 5", [[0, 5, 1]], one, blast)
    _refused(r"pair 1: seq2\[0\] = 9", [[0], [1]], [[1], [9]], blast)
    _refused("thres 0", one, one, blast, thres=0)
    E.stdaln_check(one, one, blast, mode="global", thres=0)  # the global core has no threshold
    # the overflow rule: max_score * min(len1, len2) > 32000, local mode
    E.stdaln_check([np.zeros(32000, np.uint8)], [np.zeros(40000, np.uint8)], blast)
    _refused("32001 > 32000", [np.zeros(32001, np.uint8)], [np.zeros(40000, np.uint8)], blast)
    _refused("> 32000", [np.zeros(2910, np.uint8)], [np.zeros(2910, np.uint8)], "aa2aa")  # 11 * 2910
    # the size caps
    _refused("is past", [np.zeros((1 << 22) + 1, np.uint8)], one, blast)
    _refused("cells", [np.zeros(1024, np.uint8)], [np.zeros(40000, np.uint8)], blast, mode="global")
