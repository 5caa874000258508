"""tests/index_ref.py against a committed reference index: naive_index of the stale_alt text
(300 bp) and of its reverse must give stale_alt.bwt / .rbwt / .sa / .rsa byte for byte, and
occ4_table the restated bwt_occ4 of every row.  This pins the helper the GPU tests of
test_index_adversarial_gpu.py compare against to the reference's bytes, not to our builder."""
import os

import numpy as np
import pytest

import oracle
from tests import index_ref as R


def _bwt_file(path):
    raw = open(path, "rb").read()
    hdr = np.frombuffer(raw[:20], dtype=np.uint32)
    return int(hdr[0]), tuple(int(x) for x in hdr[1:5]), np.frombuffer(raw[20:], dtype=np.uint32)


@pytest.mark.parametrize("strand", [0, 1])
def test_naive_index_equals_reference_files(golden_dir, strand):
    pre = os.path.join(golden_dir, "stale_alt")
    codes, l_pac = oracle.read_pac(pre)
    assert l_pac == 300
    ix = R.naive_index(codes if strand == 0 else codes[::-1].copy())
    primary, L2, words = _bwt_file(pre + (".bwt", ".rbwt")[strand])
    assert ix.primary == primary and ix.L2 == L2
    assert ix.words.dtype == np.uint32 and ix.words.tobytes() == words.tobytes()
    raw = open(pre + (".sa", ".rsa")[strand], "rb").read()
    hdr, body = R.sa_file_parts(raw)
    assert len(hdr) == 7 and hdr == (primary,) + L2 + (32, 300)
    assert ix.sa[0] == 300 and ix.sa[32::32].tobytes() == body.tobytes()
    # whole file images
    assert np.array((ix.primary,) + ix.L2, np.uint32).tobytes() + ix.words.tobytes() == \
        open(pre + (".bwt", ".rbwt")[strand], "rb").read()
    assert np.array(hdr, np.uint32).tobytes() + ix.sa[32::32].tobytes() == raw


@pytest.mark.parametrize("strand", [0, 1])
def test_occ4_table_equals_restated_bwt_occ4(golden_dir, strand):
    pre = os.path.join(golden_dir, "stale_alt")
    codes, _ = oracle.read_pac(pre)
    ix = R.naive_index(codes if strand == 0 else codes[::-1].copy())
    b = oracle.Bwt(pre + (".bwt", ".rbwt")[strand])
    tab = R.occ4_table(ix.bwt, ix.primary, 300)
    ks = R.occ4_ks(300)
    assert tab.shape == (302, 4) and ks[0] == 0xFFFFFFFF and ks[-1] == 300
    for k, row in zip(ks, tab):
        assert b.occ4(int(k)) == tuple(int(x) for x in row), int(k)


def test_text_family_is_what_the_gpu_tests_assume():
    """The properties the family is built for hold on the naive indexes themselves."""
    assert max(c.size for _, c in R.TEXTS) <= 8200
    a = R.text_index("A4096", 0)
    assert a.primary == 4096 and a.L2 == (4096, 4096, 4096, 4096)      # primary == n, three empty ranges
    assert R.text_index("T129", 0).L2 == (0, 0, 0, 129)
    assert R.text_index("AC4096", 0).L2[1:] == (4096, 4096, 4096)
    g = R.text_index("lastG1000", 0)
    assert g.L2[2] - g.L2[1] == 1
    # the long duplicate: the two copies share exactly DUP_UNIT symbols at their starts
    d = R.text("dup1500")
    assert d.size == 2 * R.DUP_UNIT + 37 and (d[:R.DUP_UNIT] == d[-R.DUP_UNIT:]).all()
    for nm, c in R.TEXTS:
        for s in (0, 1):
            ix = R.text_index(nm, s)
            assert ix.L2[3] == c.size and 1 <= ix.primary <= c.size
            assert ix.words.size == (c.size + 127) // 128 * 4 + 4 + (c.size + 15) // 16
