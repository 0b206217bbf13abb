"""CPU: the cases of tests/gemm_cases.py cover what the shipped plan tables run, and their checks can tell right from wrong.

Needs the built libraries' host-only queries only (df_test_gemm_key, df_test_gemm_valid), no GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import gemm_cases as G
from diff_foley_amd import engine as E

TUNED = os.path.join(os.path.dirname(os.path.abspath(E.__file__)), "tuned")
SKS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)        # csrc/engine_tune.hip autotune_plan

# (form, tile, split-K) triples of a table that only a production-size shape reaches: (precision, form, tile, split-K): reason.
# At most 5 % of a table's distinct triples, never a whole form, never a whole tile family of a form.
EXEMPT = {}


def form_of(key):
    M, N, K, taps, stride, ups, batch, geglu, e = re.fullmatch(r"(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_(\d+)_e(\d+)", key).groups()
    return int(taps), int(stride), int(ups), int(batch) > 1, int(geglu), int(e)


def shipped(prec):
    """{form: {(tile, split-K)}} of one table"""
    out = {}
    with open(os.path.join(TUNED, f"gfx950_256cu_{prec}.txt")) as fh:
        for line in fh:
            key, tile, sk, _gm = line.split()
            out.setdefault(form_of(key), set()).add((int(tile), int(sk)))
    return out


def tuner_pairs(L, d, batch):
    n_tiles = len(E.gemm_tiles(L))
    out = set()
    for t in range(n_tiles):
        for sk in SKS:
            v = L.df_test_gemm_valid(C.byref(d), t, batch, sk)
            assert v >= 0, L.df_last_error()
            if not v:
                if sk > 1:
                    break
                continue
            out.add((t, sk))
    return out


_built = {}


def case(name, prec):
    if (name, prec) not in _built:
        _built[(name, prec)] = G.CASES[name](prec)
    return _built[(name, prec)]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_cases_cover_every_shipped_form_tile_and_splitk(prec):
    """Every form of the shipped table has a case, and every (form, tile, split-K) triple the table ships is among the pairs the
    autotuner would launch for some case of that form -- so tests/test_gemm_forms_gpu.py judges it element by element.  A regenerated
    table that picks a triple no case reaches fails here until a case is added or resized (or, for a triple that needs a
    production-size shape, listed in EXEMPT with its reason)."""
    L = E.lib(prec)
    table = shipped(prec)
    reach = {}
    for name in G.CASES:
        cs = case(name, prec)
        d = cs.host_desc()
        reach.setdefault(form_of(cs.key(L)), set()).update(tuner_pairs(L, d, cs.batch))
    no_case = sorted(f for f in table if f not in reach)
    assert not no_case, f"[{prec}] forms of the shipped table without a case: {no_case}"
    fam = {t: r["family"] for t, r in E.gemm_tiles(L).items()}
    missing, exempt_used = [], []
    for f, triples in sorted(table.items()):
        for t, sk in sorted(triples):
            if (t, sk) in reach[f]:
                continue
            (exempt_used if (prec, f, t, sk) in EXEMPT else missing).append((f, t, sk))
    assert not missing, f"[{prec}] {len(missing)} shipped (form, tile, split-K) triples no case reaches: {missing}"
    total = sum(len(v) for v in table.values())
    assert len(exempt_used) * 20 <= total, f"[{prec}] {len(exempt_used)} exemptions for {total} triples"
    for f, t, sk in exempt_used:
        same_family = {(t2, s2) for t2, s2 in table[f] if fam[t2] == fam[t]}
        assert any((f, t2, s2) not in exempt_used for t2, s2 in same_family), f"[{prec}] {f}: the whole {fam[t]} family is exempt"


def _first_rows(cs, outs, clean):
    """{output: rows (first dimension of what check() compares) where outs differs from clean}"""
    rows = {}
    for k in outs:
        a, b = (outs[k][0], clean[k][0]) if k == "C" and cs.batch == 1 else (outs[k], clean[k])
        diff = ~((a.double() == b.double()) | (torch.isnan(a.double()) & torch.isnan(b.double())))
        idx = diff.reshape(diff.shape[0], -1).any(1).nonzero().flatten().tolist()
        if idx:
            rows[k] = set(idx)
    return rows


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(G.CASES))
def test_checks_pass_fp32_arithmetic_and_report_each_defect(name, prec):
    """Passes: an independent fp32 computation of the same operands (torch fp32 matmul / conv, K summed in 64-wide chunks last chunk
    first, the epilogue in fp32) goes through the case's check as if it were a kernel's output -- the bounds are not tighter than
    fp32 arithmetic allows.  Fails: each single-site defect of the case (gemm_cases._add_mutants) is reported, in a row it touched."""
    cs = case(name, prec)
    stand_in = cs.pack(cs.epi(cs.accumulate(torch.float32, chunked=True), torch.float32))
    fails, worst, _ = cs.check(stand_in)
    assert not fails and worst <= 1.0, f"{name} [{prec}]: fp32 arithmetic fails the check ({worst:.3f} x bound): {fails[:5]}"
    clean = cs.pack(cs.r["ref"])
    fails, _, _ = cs.check(clean)
    assert not fails, f"{name} [{prec}]: the reference fails its own check: {fails[:5]}"
    for label, make in cs.mutants:
        outs = make()
        touched = _first_rows(cs, outs, clean)
        assert touched, f"{name}: defect '{label}' changes nothing"
        fails, _, rows = cs.check(outs)
        assert rows, f"{name} [{prec}]: defect '{label}' passes the check"
        for what, row in rows:
            k = what.split()[0]
            assert row in touched.get(k, ()), f"{name} [{prec}]: defect '{label}' reported at {what} row {row}, it touched {touched}"


def test_every_listed_defect_has_a_case():
    """The defects of the issue's list are each injected into at least one case."""
    labels = {label for name in G.CASES for label, _ in case(name, "bf16").mutants}
    assert len(labels) >= 10, labels
