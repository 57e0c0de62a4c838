"""Host test of the pivot push's index math (conflux_amd/csrc/pivot_push.hpp):
a stand-alone program built with hipcc's host clang++ (no GPU code) runs
lists() and apply() on every case written here, and the results are checked
against a naive model in numpy.

The model holds the array of row ids at the local positions and applies the
kernels' three moves in order with the lists the program produced: gather
the pivot rows, copy each early row to the matching late position, place the
pivot rows at [f, f + cnt).  That must give exactly the gri the program
produced; igri must be its inverse on the rows held and -1 elsewhere; early
is ascending, late ascending and unique, and the two counts agree.  A
repeated pivot row must be reported as the invariant error, with counts that
stay inside the arrays and the maps untouched.

Cases: Ml in {8, 64, 257}, v in {4, 32}, cnt in {1, 3, v} (cnt < v is a rank
row of a Px > 1 grid: the ids are those of rank row 1 of 2, so igri has rows
it does not hold), every f from 0 to Ml - cnt, and per (Ml, cnt, f) the
patterns that fit: pivots in the window in order, in the window permuted,
all beyond the window, a mix, and a repeated row.  f = Ml - cnt is the
window that ends exactly at Ml.
"""
import os
import subprocess

import numpy as np
import pytest

from test_norm1est_host import _host_clangxx

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "conflux_amd", "csrc")
OK, EINVARIANT = 0, 2


def _gri(Ml, v):
    """Row ids of rank row 1 of a Px = 2 grid, tile-cyclic, then shuffled as
    earlier steps would have left them."""
    i = np.arange(Ml)
    ids = (i // v * 2 + 1) * v + i % v
    return np.random.default_rng(Ml * 100 + v).permutation(ids)


def _cases():
    """(name, Ml, M, f, cnt, pos, gri, expect)"""
    out = []
    for Ml in (8, 64, 257):
        for v in (4, 32):
            gri = _gri(Ml, v)
            M = int(gri.max()) + 1 + v
            for cnt in sorted({1, 3, v}):
                if cnt > Ml:
                    continue
                rng = np.random.default_rng(Ml * 1000 + v * 10 + cnt)
                for f in range(0, Ml - cnt + 1):
                    win = np.arange(f, f + cnt)
                    beyond = np.arange(f + cnt, Ml)
                    pats = [("inorder", win, OK),
                            ("permuted", rng.permutation(win), OK)]
                    if len(beyond) >= cnt:
                        pats.append(("beyond", rng.choice(
                            beyond, cnt, replace=False), OK))
                    if len(beyond) >= 1 and cnt >= 2:
                        nb = min(len(beyond), cnt // 2 + 1)
                        mix = np.concatenate([
                            rng.choice(win, cnt - nb, replace=False),
                            rng.choice(beyond, nb, replace=False)])
                        pats.append(("mix", rng.permutation(mix), OK))
                        rep = mix.copy()
                        rep[0] = rep[-1]  # one row twice, another missing
                        pats.append(("repeated", rep, EINVARIANT))
                    for name, pos, expect in pats:
                        out.append((f"{name} Ml={Ml} v={v} cnt={cnt} f={f}",
                                    Ml, M, f, cnt, pos.astype(np.int32),
                                    gri.astype(np.int32), expect))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("pivot_push_host")
    exe = str(d / "pivot_push_host_main")
    subprocess.run([_host_clangxx(), "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(HERE, "pivot_push_host_main.cpp"), "-o", exe],
                   check=True)
    cases = _cases()
    inp, outp = str(d / "cases.bin"), str(d / "out.bin")
    write_cases(inp, cases)
    subprocess.run([exe, inp, outp], check=True)
    return cases, read_results(outp, cases)


def write_cases(path, cases):
    with open(path, "wb") as fh:
        np.array([len(cases)], "<i4").tofile(fh)
        for _, Ml, M, f, cnt, pos, gri, _ in cases:
            np.array([Ml, M, f, cnt], "<i4").tofile(fh)
            pos.astype("<i4").tofile(fh)
            gri.astype("<i4").tofile(fh)


def read_results(path, cases):
    raw = np.fromfile(path, "<i4")
    got, at = [], 0
    for _, Ml, M, _, cnt, _, _, _ in cases:
        take = []
        for n in (3, cnt, cnt, Ml, M):
            take.append(raw[at:at + n])
            at += n
        got.append(take)
    assert at == len(raw)
    return got


def test_the_patterns_are_all_there(results):
    cases, _ = results
    names = {c[0].split()[0] for c in cases}
    assert names == {"inorder", "permuted", "beyond", "mix", "repeated"}
    # the window that ends exactly at Ml, and a full-width step
    assert any(f + cnt == Ml for _, Ml, _, f, cnt, *_ in cases)
    assert any(cnt == 32 and Ml == 257 for _, Ml, _, _, cnt, *_ in cases)


def test_lists_and_maps_against_the_three_moves(results):
    cases, got = results
    seen = 0
    for (name, Ml, M, f, cnt, pos, gri0, expect), g in zip(cases, got):
        (status, n_early, n_late), early, late, gri, igri = g
        if expect != OK:
            continue
        assert status == OK, name
        assert n_early == n_late, name
        early, late = early[:n_early], late[:n_late]
        assert np.all(np.diff(early) > 0), name
        assert np.all(np.diff(late) > 0), name  # ascending and unique
        assert np.all((early >= f) & (early < f + cnt)), name
        assert np.all((late >= f + cnt) & (late < Ml)), name
        if name.startswith(("inorder", "permuted")):
            assert n_early == 0, name
        if name.startswith("beyond"):
            assert n_early == cnt, name
        # the kernels' three moves on the row ids
        rows = gri0.copy()
        staged = rows[pos]
        rows[late] = rows[early]
        rows[f:f + cnt] = staged
        assert np.array_equal(rows, gri), name
        # what the push is for, and nothing lost
        assert np.array_equal(gri[f:f + cnt], gri0[pos]), name
        assert np.array_equal(np.sort(gri), np.sort(gri0)), name
        assert np.array_equal(gri[:f], gri0[:f]), name
        inv = np.full(M, -1, np.int32)
        inv[gri] = np.arange(Ml)
        assert np.array_equal(igri, inv), name
        seen += 1
    assert seen > 1000


def test_a_repeated_row_is_the_invariant_error(results):
    cases, got = results
    seen = 0
    for (name, Ml, M, f, cnt, pos, gri0, expect), g in zip(cases, got):
        (status, n_early, n_late), early, late, gri, igri = g
        if expect != EINVARIANT:
            continue
        assert status == EINVARIANT, name
        assert n_early != n_late, name
        assert 0 <= n_early <= cnt and 0 <= n_late <= cnt, name
        assert np.all(early[n_early:] == -1), name
        assert np.all(late[n_late:] == -1), name
        assert np.array_equal(gri, gri0), name  # the maps were left alone
        seen += 1
    assert seen > 100
