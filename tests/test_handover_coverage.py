"""The hand-over case table (tests/handover_cases.py) against the library's instantiation list, without a GPU: every
KChirpColFwd<n, false> that can take the tree's root has an eligible case, every eligible case really ends its tree in
KColInv<n> and drops it from the transform, and every ineligible case is ineligible for the reason it states.  The
schedules are the emulator's (schedule-only mode: the product's own host code, nothing executed)."""
import ctypes as C
import re

import pytest

import handover_cases as HC
from fnft_amd.capi import CSTYPE, NSE_DISC
from test_emu_kernels import emu, kernel_list  # noqa: F401  (module fixture: builds and loads tests/emu/libfnft_emu.so)


def _names(buf):
    return [n.replace(" ", "") for n in buf.value.decode().split("\n") if n]


def tree_schedule(emu, c):  # noqa: F811
    """The plan's tree alone (M = 0: nothing to hand the root to), then the export."""
    emu.emu_tree_schedule.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    assert emu.emu_tree_schedule(1, c["D"], NSE_DISC[c["disc"]], c["batch"], 0, buf, len(buf)) == 0, c["id"]
    return _names(buf)


def transform_schedule(emu, c):  # noqa: F811
    """The plan's transform (run_front, run_tree, run_contspec) with the switch at its default, on."""
    emu.emu_chirp_schedule.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                       C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    rc = emu.emu_chirp_schedule(2, c["D"], c["M"], NSE_DISC[c["disc"]], c["batch"], CSTYPE[c["cstype"]], 0, buf,
                                len(buf))
    assert rc == 0, (c["id"], rc)
    return _names(buf)


def test_handover_case_ids_unique():
    ids = HC.ids(HC.CASES)
    assert len(ids) == len(set(ids))


def uncovered(lengths, cases):
    """The column lengths of `lengths` without an eligible case whose tree and chirp both run at that length."""
    have = {c["N1"] for c in cases if c["eligible"] and c["N1"] == c["tree_n1"]}
    return sorted(set(lengths) - have)


def test_handover_coverage(emu):  # noqa: F811
    """A column length added to FA_LIST_CHIRP_N1 fails here until the table has an eligible case for it."""
    inst = {int(m.group(1)) for n in kernel_list(emu) for m in [re.fullmatch(r"KChirpColFwd<(\d+),false>", n)] if m}
    assert len(inst) == 13, sorted(inst)
    assert set(HC.EXCLUDED) <= inst, sorted(set(HC.EXCLUDED) - inst)
    need = inst - set(HC.EXCLUDED)
    assert not uncovered(need, HC.CASES), uncovered(need, HC.CASES)
    # the check can fail: without the cases of one length, that length is reported
    assert uncovered(need, [c for c in HC.CASES if c["N1"] != 64]) == [64]
    # an exclusion that a case reaches is stale
    assert not [c["id"] for c in HC.CASES if c["eligible"] and c["N1"] in HC.EXCLUDED]
    # what the table asks for besides: every deg0, kappa = -1 at an LDS column length, every contspec type
    el = [c for c in HC.CASES if c["eligible"]]
    assert {HC.DEG0[c["disc"]] for c in el} >= {1, 2, 4}
    assert [c for c in el if c["kappa"] == -1 and c["N1"] >= 32]
    assert {c["cstype"] for c in el} == set(HC.CSLEN)


@pytest.mark.parametrize("case", HC.CASES, ids=HC.ids(HC.CASES))
def test_handover_case_schedule(emu, case):  # noqa: F811
    c = case
    tree = tree_schedule(emu, c)
    cols = [n for n in tree if n.startswith("KColInv<")]
    inv = "KColInv<%d>" % c["tree_n1"]
    # the tree ends in the inverse column pass of the case's length (then the finalize and the export)
    assert cols and cols[-1] == inv and tree[-3:] == [inv, "KFinalizeScales", "KExportTm"], tree
    names = transform_schedule(emu, c)
    chirp = {int(m) for n in names for m in re.findall(r"^KChirpCol(?:Fwd|Inv)<(\d+),", n)}
    assert chirp == {c["N1"]}, names
    assert HC.failing(c) == ({c["why"]} if c["why"] else set()), (c["id"], HC.failing(c))
    if c["eligible"]:
        assert c["tree_n1"] == c["N1"] and c["D"] * HC.DEG0[c["disc"]] == c["N1"] * HC.ROW_TREE
        assert inv not in names and "KFinalizeScales" not in names, names
        assert HC.MIN_M <= c["M"] <= c["D"] * HC.DEG0[c["disc"]]
    else:
        # nothing is handed over: the transform is the tree (without its finalize, which rides on the chirp) and the chirp
        assert names[:len(tree) - 2] == tree[:-2], (names, tree)
        # the stated reason is the cause: with that one thing changed (handover_cases.flipped) the plan hands the root over
        f = HC.flipped(c)
        assert not HC.failing(f), (f, HC.failing(f))
        ftree = [n for n in tree_schedule(emu, f) if n.startswith("KColInv<")]
        assert ftree and ftree[-1] not in transform_schedule(emu, f), f
