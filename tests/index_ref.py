"""A plain reference for the FM-index, for tests only: numpy and the standard library, nothing
from ibwa_amd and no device.

naive_index() sorts the suffixes of T$ by comparing byte slices and lays the BWT out as the
reference's .bwt body; occ4_table() counts by cumulative sum.  tests/test_index_ref.py pins both
strands of a committed reference index (stale_alt.*) to these functions byte for byte, so what the
GPU tests compare against is the reference's output and not the builder under test.

TEXTS is the family of repetitive, tiny and edge-length texts of tests/test_index_adversarial_gpu.py;
every text has n <= 8200 so the naive sort stays well under a second.
"""
import functools
from typing import NamedTuple

import numpy as np

MINUS1 = 0xFFFFFFFF


class NaiveIndex(NamedTuple):
    primary: int
    L2: tuple          # L2[1..4]: cumulative symbol counts
    words: np.ndarray  # uint32, the .bwt body: per 128 symbols 4 running counts + <= 8 words, then 4 final counts
    sa: np.ndarray     # uint32[n + 1], suffix array of T$ ($ smallest): sa[0] == n
    bwt: np.ndarray    # uint8[n], the BWT with the $ row removed


def suffix_array(codes):
    """Suffix array of T$ with $ smaller than every base: sort by the byte slices of codes + 1
    (a suffix that is a prefix of another sorts first, as with $)."""
    b = (np.asarray(codes, dtype=np.uint8) + 1).tobytes()
    return np.array(sorted(range(len(b) + 1), key=lambda i: b[i:]), dtype=np.uint32)


def pack_body(bwt):
    """16 symbols per word, MSB first, then interleaved with the running counts every 128 symbols."""
    n = bwt.size
    n_words = (n + 15) // 16
    pad = np.zeros(n_words * 16, dtype=np.uint32)
    pad[:n] = bwt
    shifts = (2 * (15 - np.arange(16))).astype(np.uint32)
    packed = (pad.reshape(n_words, 16) << shifts).sum(axis=1).astype(np.uint32)
    onehot = (bwt[:, None] == np.arange(4)[None, :]).astype(np.uint32)
    out = []
    for b in range((n + 127) // 128):
        out.append(onehot[:b * 128].sum(axis=0).astype(np.uint32))
        out.append(packed[b * 8:min(b * 8 + 8, n_words)])
    out.append(onehot.sum(axis=0).astype(np.uint32))
    return np.concatenate(out).astype(np.uint32)


def naive_index(codes):
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.size
    assert 1 <= n <= 8200 and int(codes.max()) < 4
    sa = suffix_array(codes)
    primary = int(np.flatnonzero(sa == 0)[0])
    rows = np.delete(sa, primary).astype(np.int64)
    bwt = codes[rows - 1]
    cnt = np.bincount(bwt, minlength=4)
    L2 = tuple(int(x) for x in np.cumsum(cnt))
    return NaiveIndex(primary, L2, pack_body(bwt), sa, bwt)


def occ4_ks(n):
    """Every row a rank query can be asked for: -1, then 0 .. n."""
    return np.concatenate([[MINUS1], np.arange(n + 1)]).astype(np.uint32)


def occ4_table(codes_bwt, primary, n):
    """The four counts of occ4_ks(n), one row each: 0 for k == -1; k >= primary looks at k - 1
    (the $ row holds no base); the counts are those of BWT'[0 .. k] inclusive."""
    codes_bwt = np.asarray(codes_bwt, dtype=np.uint8)
    assert codes_bwt.size == n and 1 <= primary <= n
    cum = np.cumsum(codes_bwt[:, None] == np.arange(4)[None, :], axis=0).astype(np.uint32)
    k = np.arange(n + 1)
    kk = np.where(k >= primary, k - 1, k)
    return np.concatenate([np.zeros((1, 4), np.uint32), cum[kk]])


def sa_file_parts(raw):
    """A .sa / .rsa file -> (7 header words: primary, L2[1..4], sa_intv, seq_len; the sampled body)."""
    return tuple(int(x) for x in np.frombuffer(raw[:28], dtype=np.uint32)), np.frombuffer(raw[28:], dtype=np.uint32)


# ---------------------------------------------------------------- the text family

EDGE_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 20, 21, 22, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                2047, 2048, 2049)
EDGE_SINGLE = (1, 16, 32, 128, 256)
DUP_UNIT = 1500


def _periodic(unit, n):
    return np.tile(np.asarray(unit, dtype=np.uint8), n // len(unit) + 1)[:n].copy()


def _fibonacci(n):
    a, b = [0], [0, 1]
    while len(b) < n:
        a, b = b, b + a
    return np.array(b[:n], dtype=np.uint8)


def _make_texts():
    rng = np.random.default_rng(20240611)
    t = []
    # single base: LCP n - 1 (9 sort rounds at 4096), primary == n, three empty L2 ranges
    t.append(("A4096", np.zeros(4096, np.uint8)))
    t.append(("T129", np.full(129, 3, np.uint8)))
    # short periods, around the round-1 key width of 21 symbols
    t.append(("AC2049", _periodic([0, 1], 2049)))
    t.append(("per3_2048", _periodic([2, 0, 3], 2048)))
    for p in (21, 22, 23):
        t.append((f"per{p}_4097", _periodic(rng.integers(0, 4, p), 4097)))
    t.append(("fib4181", _fibonacci(4181)))
    # long duplicate: two tied groups of DUP_UNIT suffixes survive 7 rounds (21 * 2^6 < 1500 <= 21 * 2^7)
    u = rng.integers(0, 4, DUP_UNIT).astype(np.uint8)
    t.append(("dup1500", np.concatenate([u, rng.integers(0, 4, 37).astype(np.uint8), u])))
    # edge lengths: 16 symbols per word, 32 per SA sample, 128 per Occ block
    for n in EDGE_LENGTHS:
        t.append((f"rand{n}", rng.integers(0, 4, n).astype(np.uint8)))
    for n in EDGE_SINGLE:
        t.append((f"A{n}", np.zeros(n, np.uint8)))
    # skewed alphabets: two empty L2 ranges; a symbol that occurs once, at the very end
    t.append(("AC4096", rng.integers(0, 2, 4096).astype(np.uint8)))
    g = rng.choice(np.array([0, 1, 3], np.uint8), 1000)
    g[-1] = 2
    t.append(("lastG1000", g))
    return t


TEXTS = _make_texts()
TEXT_NAMES = [nm for nm, _ in TEXTS]
_BY_NAME = dict(TEXTS)
assert len(_BY_NAME) == len(TEXTS)


def text(name):
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def text_index(name, strand):
    """naive_index of the text (strand 0) or of its reverse (strand 1: the .rbwt); computed once."""
    c = _BY_NAME[name]
    return naive_index(c if strand == 0 else c[::-1].copy())
