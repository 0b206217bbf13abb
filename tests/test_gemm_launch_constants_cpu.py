"""CPU: the launch constants launch_gemm hands the GEMM-family kernels (csrc/gemm.h GemmLaunch, gemm_launch_consts in gemm.hip).

The kernels' prologues divide by nothing: tile counts, the tile walk, the K range of a split and the halo geometry come from the
host, and what is still divided on the device goes through a multiply-high magic number (block-uniform quotients and conv rows:
x / d == umulhi(x, mul) >> sh below 2^31) or a reciprocal (the halo kernels' per-thread quotients, FastDiv: trunc((x + 0.5) * inv),
inv = 1.0f / (float)d, below 2^22) that the host computed.  df_test_gemm_launch_constants (host only) returns the constants of a
descriptor; the device's use of them is restated here in numpy uint64 / float32 arithmetic (tile_of_lc, magic_div, FastDiv::div of
csrc/gemm_impl.h) and held against the plain integer formulas the kernels used to evaluate themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gemm_cases as G
from diff_foley_amd import engine as E
from test_gemm_cases_cpu import TUNED, case, tuner_pairs

F32 = np.float32
GMS = (0, 1, 2, 4, 8, 16)           # the walk orders autotune_plan tries
LIM = 1 << 22                       # FastDiv is exact for 0 <= x < 2^22; gemm_route refuses what would pass it


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not all(os.path.exists(p) for p in E.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()


@pytest.fixture(params=["bf16", "fp16"])
def L(request):
    return E.lib(request.param)


def consts(L, d, tile, sk=1, batch=1):
    """The launch constants of (d, tile, batch, sk), or None where launch_gemm refuses the problem."""
    out = E.GemmLaunch(size=C.sizeof(E.GemmLaunch))
    rc = L.df_test_gemm_launch_constants(C.byref(d), tile, batch, sk, C.byref(out))
    assert rc in (0, 2), L.df_last_error()
    return out if rc == 0 else None


def fdiv(x, inv):
    """FastDiv::div on an int array: float32 throughout, as the device evaluates it"""
    return ((x.astype(F32) + F32(0.5)) * F32(inv)).astype(np.int64)


def mdiv(x, m):
    """magic_div on an int array; m = (mul, sh, d)"""
    mul, sh, d = m
    return x if d == 1 else (x.astype(np.uint64) * np.uint64(mul) >> np.uint64(32 + sh)).astype(np.int64)


def magic(c, name):
    m = c.magic[E.GemmLaunch.MAGIC.index(name)]
    return m.mul, m.sh, m.d


def walk_device(c, bid):
    """tile_of_lc: block id -> (mt, nt) from the constants alone"""
    xcd, idx = bid & 7, bid >> 3
    lid = np.where(xcd < c.xr, xcd * (c.xq + 1), c.xr * (c.xq + 1) + (xcd - c.xr) * c.xq) + idx
    per, rows, last = magic(c, "per"), magic(c, "rows"), magic(c, "last")
    grp = mdiv(lid, per)
    rem = lid - grp * per[2]
    full = c.nbm - grp * c.gm >= c.gm
    nt = np.where(full, mdiv(rem, rows), mdiv(rem, last))
    return grp * c.gm + (rem - nt * np.where(full, rows[2], last[2])), nt


def walk_plain(nbm, nbn, gm, bid):
    """The XCD remap and tile_of with plain integer division"""
    nblk = nbm * nbn
    q, r, xcd, idx = nblk >> 3, nblk & 7, bid & 7, bid >> 3
    lid = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + idx
    if gm <= 0 or gm >= nbm:
        return lid % nbm, lid // nbm
    per = gm * nbn
    grp = lid // per
    rem = lid - grp * per
    rows = np.minimum(gm, nbm - grp * gm)
    nt = rem // rows
    return grp * gm + (rem - nt * rows), nt


def test_tile_map(L):
    """Every nbm in 1 .. 40 x nbn in 1 .. 12 x gm in {0, 1, 2, 3, 5, 8, nbm, nbm + 1}, every block id: (mt, nt) from the host constants
    is the plain division formula's, and the map is a bijection onto the tiles.  Tile 3 (64 x 64); the halo and wide tiles share
    the function, with their own nbm."""
    for nbm in range(1, 41):
        for nbn in range(1, 13):
            bid = np.arange(nbm * nbn, dtype=np.int64)
            for gm in sorted({0, 1, 2, 3, 5, 8, nbm, nbm + 1}):
                d = E.GemmDesc(M=64 * nbm - 7, N=64 * nbn - 4, K=64)
                d.gm = gm
                c = consts(L, d, 3)
                assert (c.nbm, c.nbn, c.nblk, c.xq, c.xr) == (nbm, nbn, nbm * nbn, nbm * nbn >> 3, nbm * nbn & 7)
                ge = nbm if gm <= 0 or gm >= nbm else gm
                assert (c.gm, magic(c, "per")[2], magic(c, "rows")[2], magic(c, "last")[2]) == (ge, ge * nbn, ge, nbm % ge or ge)
                mt, nt = walk_device(c, bid)
                pm, pn = walk_plain(nbm, nbn, gm, bid)
                assert np.array_equal(mt, pm) and np.array_equal(nt, pn), (nbm, nbn, gm)
                assert sorted(zip(mt.tolist(), nt.tolist())) == [(m, n) for m in range(nbm) for n in range(nbn)], (nbm, nbn, gm)


def test_tile_counts_of_halo_and_wide_tiles(L):
    """nbm of a halo tile counts blocks of PB patches (a batch of 3 leaves the last block short), of a wide tile rows of 64 RT."""
    for tile, (H, Wd), nb in ((23, (8, 16), 3), (24, (4, 16), 3), (25, (8, 16), 3), (5, (6, 8), 2)):
        c = consts(L, E.GemmDesc(conv=1, NB=nb, H=H, Wd=Wd, Cin=64, N=128, stride=1), tile)
        bm = E.gemm_tiles(L)[tile]["bm"]
        assert c.PPX == c.th * c.tw and c.PB == bm // c.PPX and c.HWp == (c.th + 2) * (c.tw + 2) and c.HR == c.PB * c.HWp
        assert c.npx == Wd // c.tw and c.npy == H // c.th and c.pimg == c.npx * c.npy and c.npatch == nb * H * Wd // c.PPX
        assert c.nbm == -(-c.npatch // c.PB) and c.nblk == c.nbm * c.nbn
        rpp = E.gemm_tiles(L)[tile]["dma_threads"] // 8
        assert c.APASS == -(-c.HR // rpp)
    one = (C.c_float * 4096)()
    p = C.addressof(one)
    for tile, M in ((32, 300), (33, 200), (34, 72)):
        d = E.GemmDesc(M=M, N=2560, K=320, geglu=1, A=p, W=p, C=p, ln_stats=p, ln_C=320, ln_slots=5, ln_cs=p, bias=p, out_operand=1)
        c = consts(L, d, tile)
        assert (c.nbm, c.nbn, c.nk) == (-(-M // E.gemm_tiles(L)[tile]["bm"]), 8, 5)


def test_split_k_ranges(L):
    """Every nk in 1 .. 40 x every split count 1 .. 40 the route admits: split z owns K steps [z per, min(nk, (z + 1) per)) with
    per = ceil(nk / sk) -- empty trailing splits included -- and the ranges partition [0, nk).  Halo tiles: the same over 64-channel
    slices, and the folded skip's n2tot slices dealt per2 = ceil(n2tot / used) each to the `used` splits that own conv slices."""
    one = (C.c_float * 64)()
    p = C.addressof(one)
    for nk in range(1, 41):
        for sk in range(1, 41):
            per = -(-nk // sk)
            c = consts(L, E.GemmDesc(M=64, N=64, K=64 * nk), 3, sk)
            if c is not None:
                assert (c.nk, c.kper) == (nk, per)
                got = [(z * c.kper, min(c.nk, z * c.kper + c.kper)) for z in range(sk)]
                assert got == [(z * per, min(nk, (z + 1) * per)) for z in range(sk)]
                steps = [k for a, b in got for k in range(a, b)]
                assert steps == list(range(nk)), (nk, sk)
            for cin2 in (0, 64, 192, 640):
                d = E.GemmDesc(conv=1, NB=1, H=8, Wd=16, Cin=64 * nk, N=64, stride=1, A2=p if cin2 else None, lda2=cin2, Cin2=cin2)
                c = consts(L, d, 23, sk)
                if c is None:
                    continue
                n2tot = cin2 // 64
                used = -(-nk // per)
                per2 = -(-n2tot // used)
                assert (c.nk, c.kper, c.n2tot, c.used, c.per2) == (nk, per, n2tot, used, per2)
                tail = []
                for z in range(sk):
                    s0 = z * c.per2
                    n2 = max(min(c.n2tot, s0 + c.per2) - s0, 0) if z < c.used else 0
                    assert (n2 > 0) <= (z * per < nk), "a split without conv slices got skip slices"
                    tail += list(range(s0, s0 + n2))
                assert tail == list(range(n2tot)), (nk, sk, cin2)


# ------------------------------------------------------------------------------------------------------------------------------
# every divisor the route can produce for the shapes of tests/gemm_cases.py and of the two shipped tables
_MAPS = [(16, 64), (8, 32), (4, 16), (2, 8), (32, 128), (64, 256), (128, 512), (256, 1024), (56, 56), (28, 28), (14, 14), (7, 7)]


def _table_descs(prec):
    """(descriptor, tile, split-K, gm) of every row of a shipped table.  A key names M, N, K, taps, stride, ups: a conv row is tried on
    every map of the models (_MAPS) that its M is a whole number of."""
    one = (C.c_float * 64)()
    p = C.addressof(one)
    keep = [one]
    rows = []
    with open(os.path.join(TUNED, f"gfx950_256cu_{prec}.txt")) as fh:
        for line in fh:
            key, tile, sk, gm = line.split()
            M, N, K, taps, stride, ups, batch, geglu, e = map(int, re.fullmatch(r"(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_e(\d+)", key).groups())
            ds = []
            if taps == 1:
                f = dict(M=M, N=N, K=K)
                if geglu:
                    f.update(geglu=1, A=p, W=p, C=p, ln_stats=p, ln_C=K, ln_slots=K // 64, ln_cs=p, bias=p, out_operand=1)
                ds.append(E.GemmDesc(**f))
            else:
                for H, Wd in _MAPS:
                    opix = (H * Wd * 4) if ups else (H * Wd // 4) if stride == 2 else H * Wd
                    if M % opix:
                        continue
                    c2s = [c2 for c2 in range(64, K, 64) if (K - c2) % (9 * 64) == 0] if (e & 32) else [0]
                    for c2 in c2s:
                        f = dict(conv=2 if taps == 4 else 1, NB=M // opix, H=H, Wd=Wd, Cin=(K - c2) // taps, N=N, stride=stride, ups=ups)
                        if c2:
                            f.update(A2=p, lda2=c2, Cin2=c2)
                        ds.append(E.GemmDesc(**f))
            for d in ds:
                d.gm = int(gm)
            rows.append((key, ds, int(tile), int(sk), batch))
    return rows, keep


def _divisors(L, prec):
    """{(d, inv)} of FastDiv and {(mul, sh, d)} of magic_div over the cases and the table of this build"""
    fd, mg = set(), set()

    def take(c, halo, conv):
        mg.update(magic(c, n) for n in ("per", "rows", "last"))
        if magic(c, "wrb")[2]:
            mg.add(magic(c, "wrb"))
        if conv:
            mg.update(magic(c, n) for n in ("ohw", "ow", "cin"))
        if halo:
            fd.update({(c.HWp, c.inv_hwp), (c.tw + 2, c.inv_tw2), (c.pimg, c.inv_pimg), (c.npx, c.inv_npx), (c.PPX, c.inv_ppx), (c.tw, c.inv_tw)})

    tiles = E.gemm_tiles(L)
    for name in G.CASES:
        cs = case(name, prec)
        d = cs.host_desc()
        for tile, sk in sorted(tuner_pairs(L, d, cs.batch)):
            for gm in GMS:
                d.gm = gm
                c = consts(L, d, tile, sk, cs.batch)
                assert c is not None, (name, tile, sk)
                take(c, tiles[tile]["family"] == "halo", cs.kind != "lin")
    rows, keep = _table_descs(prec)
    for key, ds, tile, sk, batch in rows:
        got = [c for c in (consts(L, d, tile, sk, batch) for d in ds) if c is not None]
        assert got, f"no descriptor of table row {key} (tile {tile}, split-K {sk}) is accepted: _MAPS lacks its map"
        for c in got:
            take(c, tiles[tile]["family"] == "halo", not key.split("_")[3] == "1")
    return fd, mg


def test_reciprocals_are_exact(L, request):
    """Every FastDiv divisor: the host's reciprocal is the IEEE 1.0f / (float)d, and div(x) == x // d at x = k d - 1, k d, k d + 1 for
    every k up to the 2^22 bound and at the bound itself.  Every magic number: x // d at the same points up to 2^31 (all k where
    there are at most 2^19 of them, else the first and the last 2^16 and 2^18 evenly spread ones) and at 2^31 - 1."""
    prec = request.node.callspec.params["L"]
    fd, mg = _divisors(L, prec)
    assert len(fd) > 10 and len(mg) > 40
    for d, inv in sorted(fd):
        assert 1 <= d < LIM
        assert F32(inv).tobytes() == (F32(1.0) / F32(d)).tobytes(), d
        k = np.arange(0, LIM // d + 1, dtype=np.int64) * d
        x = np.concatenate([k - 1, k, k + 1, [LIM - 1, LIM]])
        x = x[(x >= 0) & (x <= LIM)]
        assert np.array_equal(fdiv(x, inv), x // d), d
    top = (1 << 31) - 1
    for mul, sh, d in sorted(mg, key=lambda m: m[2]):
        assert 1 <= d <= top
        nk = top // d + 1
        k = np.arange(nk, dtype=np.int64) if nk <= (1 << 19) else np.unique(np.concatenate(
            [np.linspace(0, nk - 1, 1 << 18).astype(np.int64), np.arange(1 << 16, dtype=np.int64), np.arange(nk - (1 << 16), nk, dtype=np.int64)]))
        x = np.concatenate([k * d - 1, k * d, k * d + 1, [top]])
        x = x[(x >= 0) & (x <= top)]
        assert np.array_equal(mdiv(x, (mul, sh, d)), x // d), d
