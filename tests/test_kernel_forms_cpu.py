"""CPU: the shape tables of the norm / attention GPU tests (tests/kernel_cases.py) reach every kernel form the launchers can pick.

The form of a shape comes from the built libraries (df_test_groupnorm_form / df_test_attention_form, host only): the very
functions launch_groupnorm* and launch_attention dispatch on.  The set of forms that must be covered is DISCOVERED by sweeping
those functions over a wide grid of shapes, not written down here, so an instantiation added to a launcher later shows up in the
sweep and fails this test until kernel_cases.py has a row for it."""
import itertools
import os

import pytest

from diff_foley_amd import engine as E
import kernel_cases as KC


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not all(os.path.exists(p) for p in E.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()


@pytest.fixture(params=["bf16", "fp16"])
def L(request):
    return E.lib(request.param)


_GN_HW = sorted(set(list(range(1, 66)) + [2 ** k + d for k in range(6, 17) for d in (-1, 0, 1)] + [250, 777, 1000, 1090, 1500, 5461, 9000, 20000]))
_GN_C = [64 * k for k in range(1, 41)]


def _gn_mode_slabs(mode, nslab):
    return 0 if mode == "plain" else nslab


def test_groupnorm_cases_reach_every_form(L):
    reachable = {"plain": set(), "slabs": set()}
    for HW, C in itertools.product(_GN_HW, _GN_C):
        reachable["plain"].add(L.df_test_groupnorm_form(2, HW, C, 0))
        reachable["slabs"].add(L.df_test_groupnorm_form(2, HW, C, 3))
    reachable["own"] = reachable["slabs"]          # both slab paths go through the same choice
    # the sweep itself finds what the launcher's source shows: nine register forms, streaming and chunked without slabs
    assert reachable["plain"] == set(KC.GN_FORMS_REG) | {KC.GN_STREAMING, KC.GN_CHUNKED}
    assert reachable["slabs"] == set(KC.GN_FORMS_REG) | {KC.GN_REFUSED}
    for mode in ("plain", "slabs", "own"):
        got = {L.df_test_groupnorm_form(N, HW, C, _gn_mode_slabs(m, nslab)) for m, N, HW, C, _s, _e, nslab, _c in KC.GN_CASES if m == mode}
        want = reachable[mode] - {KC.GN_REFUSED}
        assert got == want, f"GroupNorm {mode}: forms without a case {sorted(want - got)}, unexpected {sorted(got - want)}"


def test_groupnorm_cases_hold_what_the_tests_promise(L):
    cases = KC.GN_CASES
    for mode in ("plain", "slabs", "own"):
        shapes = {(HW, C) for m, _n, HW, C, *_ in cases if m == mode}
        assert {(256, 320), (256, 960), (1024, 640), (1024, 960)} <= shapes, mode      # what the shipped model runs on a 16 x 64 latent
    # a pass count that does not divide HW, for every register form with more than one pass, in every mode
    for mode in ("plain", "slabs", "own"):
        ragged = set()
        for m, N, HW, C, _s, _e, nslab, _c in cases:
            per = L.df_test_groupnorm_form(N, HW, C, _gn_mode_slabs(m, nslab))
            if m == mode and per > 1 and HW % per:
                ragged.add(per)
        assert ragged == set(KC.GN_FORMS_REG) - {1}, (mode, ragged)
    # the streaming kernel on more than 16384 items with C not 128 / 256 / 512; both block orders of the register kernel
    assert any(L.df_test_groupnorm_form(N, HW, C, 0) == KC.GN_STREAMING and HW * (C // 64) > 16384 and C not in (128, 256, 512)
               for m, N, HW, C, *_ in cases if m == "plain")
    assert {N % 8 == 0 for _m, N, *_ in cases} == {True, False}
    # nothing larger than the (1, 65536, 128) case of tests/test_kernels_gpu.py
    assert max(N * HW * C * max(nslab, 1) for _m, N, HW, C, _s, _e, nslab, _c in cases) <= KC.GN_MAX_ELEMS == 65536 * 128
    for m, N, HW, C, _s, _e, nslab, c_own in cases:
        assert (m == "plain") == (nslab == 0) and (m == "own") == (c_own > 0) and c_own % 2 == 0 and c_own <= C


def test_layernorm_cases_reach_every_width():
    assert {C for _r, C, _ld in KC.LN_CASES} == {64 * nv for nv in range(1, 33)}
    assert {ld > C for _r, C, ld in KC.LN_CASES} == {True, False} and all(ld >= C for _r, C, ld in KC.LN_CASES)
    rows = {r for r, _c, _ld in KC.LN_CASES}
    assert 1 in rows and any(r % 4 == 0 for r in rows) and any(r % 4 for r in rows if r > 4)


def test_attention_cases_reach_every_form(L):
    dims = [D for D in range(1, 257) if L.df_test_attention_form(D, 64, 64)]
    assert tuple(dims) == KC.ATTN_DIMS
    reachable = {(D, L.df_test_attention_form(D, Tq, Tk)) for D in dims for Tq in range(1, 300) for Tk in (1, 31, 32, 33, 64, 96, 128, 200)}
    assert {f for _d, f in reachable} == set(KC.ATTN_FORMS)
    covered = lambda cases: {(D, L.df_test_attention_form(D, Tq, Tk)) for _n, _h, D, Tq, Tk, _f in cases}
    got = covered(KC.ATTN_CASES)
    assert got == reachable, f"attention (D, form) pairs without a case: {sorted(reachable - got)}"
    # the fused [M][2C] layout reaches every pair as well
    assert covered([c for c in KC.ATTN_CASES if c[5]]) == reachable
    block = {66: 128, 65: 128, 33: 64, 17: 32}
    for D in dims:
        for form in (66, 65, 33):
            mine = [(Tq, Tk) for _n, _h, d, Tq, Tk, _f in KC.ATTN_CASES if d == D and L.df_test_attention_form(d, Tq, Tk) == form]
            if (D, form) not in reachable:
                assert not mine
                continue
            assert any(Tq % block[form] for Tq, _ in mine), (D, form, "no ragged last query block")
            if form != 66:      # <D,4,2> only takes Tk % 64 == 0
                assert any(Tk % 32 for _, Tk in mine), (D, form, "no Tk off the 32-key tile")
    assert all(Tq == Tk for _n, _h, _d, Tq, Tk, f in KC.ATTN_CASES if f)


def test_form_queries_agree_with_the_launchers_limits(L):
    """The form functions refuse what the launchers refuse: a slab input beyond the register kernel, channel counts off 64, head
    dims outside attention_supported."""
    assert L.df_test_groupnorm_form(1, 20000, 64, 2) == KC.GN_REFUSED
    assert L.df_test_groupnorm_form(1, 20000, 64, 0) == KC.GN_STREAMING
    assert L.df_test_groupnorm_form(1, 65536, 128, 0) == KC.GN_CHUNKED
    assert L.df_test_groupnorm_form(1, 16, 100, 0) == KC.GN_REFUSED
    assert L.df_test_attention_form(20, 64, 64) == 0
    assert [L.df_test_attention_form(40, tq, 64) for tq in (1, 63, 64, 127, 128)] == [17, 17, 33, 33, 66]
    assert [L.df_test_attention_form(160, tq, 64) for tq in (63, 64, 128)] == [17, 33, 65]
