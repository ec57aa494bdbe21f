"""-m "not gpu": what tests/test_chunk_attn_exact_gpu.py relies on, proved without a device -- the statement's mask equals
oracle/ops_ref.chunk_mask and the host build of csrc/chunk_geom.h in every case of the table (nglo 0 and 7 included), the fp32
restatement and the per-chunk restatement of the fused algorithm stay inside the bounds, every mutant of tests/chunk_attn_ref.MUTANTS
leaves them by a factor of at least 2 in a case the table names for it, the case -> kernel facts of the docstring are the computed ones,
and the stress cases hold their planted maxima."""
import re

import pytest
import torch

from oracle import ops_ref
from tests import chunk_attn_ref as R
from tests.test_chunk_attn_cpu import _units, geom, make_restatement  # noqa: F401  (geom: the fixture that compiles chunk_geom_host.cpp)

BF16, F32 = torch.bfloat16, torch.float32
FACTOR = 2.0  # a kernel that carried the mutant would still differ by more than 1 x the bound after its own error of at most 1 x
CASE_IDS = [c["name"] for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_mask_equals_chunk_mask_and_chunk_geom(geom, case):  # noqa: F811
    """index arithmetic == the predicate of the dense route == the slot maps of the fused kernels: every chunk's live neighbourhood slots
    are the mask row of each of its queries, every local token is an own slot of exactly one chunk, a global row sees everything"""
    nglo, nx, ny, L = case["nglo"], case["nx"], case["ny"], case["L"]
    m = R.mask(case)
    assert m.shape == (L, L) and torch.equal(m, m.t())
    assert torch.equal(m, ops_ref.chunk_mask(R.table(case)))
    assert geom.cg_t_supported(nglo, nx, ny, R.W) == 1
    assert bool(m[:nglo].all()) and bool(m[:, :nglo].all())
    seen = torch.zeros(L, dtype=torch.long)
    for own, nb in _units(geom, nglo, nx, ny):
        row = torch.zeros(L, dtype=torch.bool)
        row[torch.from_numpy(nb).long()] = True
        own = torch.from_numpy(own).long()
        assert bool((m[own] == row[None, :]).all())
        seen[own] += 1
    assert bool((seen[:nglo] == 0).all()) and bool((seen[nglo:] == 1).all())


def test_case_table_is_the_docstring(geom):  # noqa: F811
    """the case -> kernel table of chunk_attn_ref's docstring, line by line, against facts(); and what the issue's table claims of the
    cases: B != nH and never both 2, ranges full / holding one token, slot 447 live, the dead waves of `ragged`, both softmax kernels"""
    rows = {}
    for line in R.__doc__.splitlines():
        f = line.split()
        if len(f) == 13 and f[0] in R.BY_NAME:
            rows[f[0]] = f
    assert sorted(rows) == sorted(R.BY_NAME)
    for c in R.CASES:
        k = R.facts(c)
        want = [c["name"], k["grid"], k["nglo"], k["L"], k["Np"], k["hd"], k["B"], k["nH"], k["nsplit"], k["last"], k["live00"], k["dead"], k["softmax"]]
        assert rows[c["name"]] == [str(w) for w in want], (rows[c["name"]], want)
        assert c["B"] != c["nH"] and (c["B"], c["nH"]) != (2, 2)
        own, nb = _units(geom, c["nglo"], c["nx"], c["ny"])[0]
        assert len(nb) == k["live00"]
    F = {c["name"]: R.facts(c) for c in R.CASES}
    assert (F["cell"]["L"], F["cell"]["live00"]) == (2, 2)
    assert F["sub_chunk_noglo"]["nglo"] == 0 and F["max_globals"]["nglo"] == 7 and F["max_globals"]["slot447"] and F["max_globals"]["Np"] == 240
    assert F["strip"]["grid"].startswith("1x") and F["ragged"]["hd"] == 48 and F["ragged"]["dead"] == 3 * 3 + 1  # chunk row 1 is one grid row: waves 1..3 of its 3 chunks; chunk (0, 2) is one column: wave 3
    assert F["interior"]["live00"] == 1 + 14 * 14 and F["interior"]["softmax"] == "long" and F["interior"]["Np"] == 496
    assert (F["range512"]["nsplit"], F["range512"]["last"]) == (1, 512) and (F["range513"]["nsplit"], F["range513"]["last"]) == (2, 1)
    assert (F["range1025"]["nsplit"], F["range1025"]["last"]) == (3, 1) and (F["stress_513"]["nsplit"], F["stress_513"]["last"]) == (2, 1)
    # a chunk whose 441 neighbours all live exists in `interior`
    assert max(len(nb) for _, nb in _units(geom, 1, 22, 22)) == 1 + 441
    assert {k["softmax"] for k in F.values()} == {"short", "long"}


@pytest.mark.parametrize("case", [c for c in R.CASES if c["stress"]], ids=lambda c: c["name"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_name)
def test_stress_cases_hold_their_planted_maxima(case, dt):
    x = R.inputs(case, dt)
    q, k, _ = R.heads(x["qkv"], case, 3)
    S = x["scale"] * (q @ k.transpose(-1, -2))  # [B, nH, L, L]
    m = R.mask(case)
    Sm = S.masked_fill(~m, float("-inf"))
    assert float(S.std()) > 0.5 * R.ALIGN
    for (img, qi, kj, _, score, what) in R.plants(case):
        for h in range(case["nH"]):
            if score == R.PLANT_OUT:
                assert not m[qi, kj] and int(S[img, h].argmax()) == qi * case["L"] + kj, what
            else:
                assert m[qi, kj] and int(Sm[img, h, qi].argmax()) == kj, (what, h)
                assert float(Sm[img, h, qi, kj]) > 200.0, what
    # the probability the dense route must make exactly 0 is, unmasked, the whole row
    img, qi, kj = [p for p in R.plants(case) if p[4] == R.PLANT_OUT][0][:3]
    assert float(torch.softmax(S[img, 0, qi], -1)[kj]) > 0.999


def _params():
    return [(c, dt, route) for c in R.CASES for route in R.ROUTES for dt in R.DTYPES if not (route == "fused" and dt != BF16)]


@pytest.mark.parametrize("case,dt,route", _params(), ids=lambda p: p["name"] if isinstance(p, dict) else (R.dt_name(p) if isinstance(p, torch.dtype) else p))
def test_fp32_restatement_is_inside_the_bounds(case, dt, route):
    """oracle/ops_ref.vit_attn_fwd / _bwd in fp32 on the same inputs: every element of every output under the final bound, and -- torch's
    exp is no __expf -- under the DERIVED bound of the dense route in fp32 as well"""
    got = R.restatement(case, dt)
    m = R.metrics(case, dt, route, got, outputs=("attn", "lse", "out", "dq", "dk", "dv"))
    if route == "dense":
        ref = R.statement(case, dt, "dense") if dt == F32 else None
        if ref is not None:
            for kk in R.OUTPUTS["dense"]:
                m["ratio_derived_" + kk] = R.ratio(got[kk], ref[kk], ref["bd_" + kk])
        assert bool((got["attn"][:, :, ~R.mask(case)] == 0).all())
    R.check("restatement_fp32", case, dt, route, m)


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_per_chunk_restatement_is_inside_the_fused_bounds(geom, case):  # noqa: F811
    """the algorithm of chunk_attn.hip restated per chunk (tests/test_chunk_attn_cpu.make_restatement: the kernels' units of work, the
    online range walk of the global rows, the saved log-sum-exp, delta from the stored out) in fp32 on the bf16 inputs"""
    x = R.inputs(case, BF16)
    B, nH, L = case["B"], case["nH"], case["L"]
    fwd, bwd = make_restatement(geom)
    lay = R.layout(case, "cpu")
    out, saved = fwd(x["qkv"].float(), B, L, nH, x["scale"], lay)
    dqkv = bwd(x["dout"].float(), saved, B, L, nH, x["scale"], lay)
    R.check("per_chunk_restatement", case, BF16, "fused", R.metrics(case, BF16, "fused", R.unpack(case, out=out, dqkv=dqkv, lse=saved[2])))


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_every_mutant_leaves_its_bound_by_the_factor(name):
    route, names, what = R.MUTANTS[name]
    best = 0.0
    for dt in ((BF16,) if route == "fused" else R.DTYPES):
        worst_dt = 0.0
        for cn in names:
            case = R.BY_NAME[cn]
            ref = R.reference(case, dt, route)
            mut = R.statement(case, dt, route, mutant=name, want_bounds=False)
            rs = {kk: R.ratio(mut[kk], ref[kk], ref["bd_" + kk]) for kk in R.OUTPUTS[route]}
            print("MUTANT", name, what, cn, R.dt_name(dt), {kk: "%.3g" % vv for kk, vv in rs.items()})
            worst_dt = max(worst_dt, max(rs.values()))
        assert worst_dt >= FACTOR, (name, what, R.dt_name(dt), worst_dt)
        best = max(best, worst_dt)
    assert best >= FACTOR


def test_mutant_table_names_only_cases_it_has():
    assert len(R.MUTANTS) == 15
    for name, (route, names, _) in R.MUTANTS.items():
        assert route in R.ROUTES and names and all(n in R.BY_NAME for n in names), name
    assert re.search(r"Fused route", R.__doc__) and re.search(r"Dense route", R.__doc__)
