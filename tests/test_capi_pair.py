"""ibwa_aln_parse_args2 (aln_opts.cpp) and its Python mirror engine.parse_aln_cmdline: the `aln`
command line with -F, the second output of the CLI's pair mode.  No GPU needed."""
import ctypes
import json
import os

import pytest

import oracle
from ibwa_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opt_bytes(o):
    return ctypes.string_at(ctypes.addressof(o), ctypes.sizeof(o))


def option_sets():
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "sai_manifest.json")))
    sets = [m["argv"] for m in man.values()]
    sets += [[], ["-n", "0.01", "-e", "0"], ["-e", "5", "-N", "-R", "7"], ["-B", "4", "-q", "20", "-I", "-c", "-L", "-m", "1000"],
             ["-b", "-1"], ["-b", "-0", "-2"], ["-t", "8", "-l", "25", "-k", "1", "-d", "5", "-i", "3"],
             ["-M", "2", "-O", "9", "-E", "3", "-o", "2"]]
    return sets


def test_cmdline_with_pair_outputs():
    args = ["-n", "3", "-f", "a", "-F", "b", "-G", "2", "p", "x", "y"]
    o, n_gpus, f1, f2, first = engine.parse_aln_cmdline(args)
    assert (f1, f2, n_gpus, first) == ("a", "b", 2, 8)
    assert args[first:] == ["p", "x", "y"]
    assert o.max_diff == 3 and o.fnr == -1.0
    assert opt_bytes(o) == opt_bytes(engine.parse_aln_args(["-n", "3"]))


def test_cmdline_without_pair_output():
    o, n_gpus, f1, f2, first = engine.parse_aln_cmdline(["-q", "15", "-f", "out.sai", "p", "x"])
    assert (n_gpus, f1, f2, first) == (1, "out.sai", None, 4)
    assert o.trim_qual == 15
    o, n_gpus, f1, f2, first = engine.parse_aln_cmdline([])
    assert (n_gpus, f1, f2, first) == (1, None, None, 0)
    assert opt_bytes(o) == opt_bytes(engine.default_opt())


@pytest.mark.parametrize("argv", option_sets(), ids=lambda a: " ".join(a) or "defaults")
def test_options_equal_old_parser_and_reference(argv):
    """Without -F the new entry point gives the gap_opt_t of ibwa_aln_parse_args byte for byte, and
    the fields of the oracle's restatement of bwa_aln's option handling (as tests/test_capi.py)."""
    new, n_gpus, f1, f2, first = engine.parse_aln_cmdline(argv)
    old = engine.parse_aln_args(argv)
    assert opt_bytes(new) == opt_bytes(old)
    assert (n_gpus, f1, f2, first) == (1, None, None, len(argv))
    exp, _ = oracle.parse_aln_args(argv)
    for f, _ in engine.GapOpt._fields_:
        assert getattr(new, f) == getattr(exp, f), (argv, f)
    # -F changes no option: the same set with both outputs named
    both, _, f1, f2, _ = engine.parse_aln_cmdline(argv + ["-f", "o1", "-F", "o2"])
    assert opt_bytes(both) == opt_bytes(old) and (f1, f2) == ("o1", "o2")


def test_old_entry_point_drops_pair_output():
    """ibwa_aln_parse_args parses -F and drops its argument, as it does -f's with fn_out NULL."""
    o = engine.parse_aln_args(["-n", "2", "-F", "x", "-f", "y"])
    assert opt_bytes(o) == opt_bytes(engine.parse_aln_args(["-n", "2"]))
    # called directly with fn_out: -f is still reported, the return value is the first positional
    argv = [b"aln", b"-F", b"x", b"-f", b"y", b"-G", b"3", b"p"]
    arr = (ctypes.c_char_p * len(argv))(*argv)
    go, n_gpus, f1 = engine.GapOpt(), ctypes.c_int(0), ctypes.c_char_p()
    rc = engine.lib().ibwa_aln_parse_args(len(argv), arr, ctypes.byref(go), ctypes.byref(n_gpus), ctypes.byref(f1))
    assert (rc, n_gpus.value, f1.value) == (7, 3, b"y")
    assert opt_bytes(go) == opt_bytes(engine.default_opt())


def test_unknown_option_still_rejected():
    with pytest.raises(engine.IbwaError):
        engine.parse_aln_cmdline(["-Z"])
    with pytest.raises(engine.IbwaError):
        engine.parse_aln_args(["-Z"])
    with pytest.raises(engine.IbwaError):
        engine.parse_aln_cmdline(["-F"])  # -F needs an argument
