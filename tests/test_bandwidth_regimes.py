"""The fp64 table path (NLE_MODE_PHI_FREE) where its bandwidth-guarded kernel forms switch.

Three host predicates in csrc/sorted.hip decide per image which form of the sorted kernels runs: `sorted_moments_ok`
(the moment form of `k_sorted_pass`), `sorted_recurrence` (column factors by recurrence, more than 12 sample columns)
and `sorted_gsum_ok` (the Gram on index sums).  Each is a bound on an exponent that keeps every intermediate inside
fp64's normal range.  The cases here sit 2 % inside and 2 % outside each bound, and at W / hx = 30 where the distance
table itself runs through the denormals to zero inside one image row; every other table-path test has W / hx <= 8.

The oracle is well posed in this range (lambda_min(Ka) > 1e-3, no eigenvalue near the 1e-10 cut), so device and oracle
are compared ELEMENT BY ELEMENT: |Y - Y_o| <= 2^-23 |Y_o| + A_REL max|Y_o[j]| on every pixel of every layer, and again
on the pixels a whole-plane norm hides (the end of every row, the neighbours of the samples, the samples themselves).
Which form ran is shown without any new entry point: the sorted kernels are bitwise reproducible, so forcing the plain
forms through the environment is a bitwise no-op exactly where the predicates had already chosen them.

`record()` computes every figure once per case; the tests assert on that record, and
`tools/bandwidth_regimes_report.py` writes the same records to `profiles/r9_bandwidth_regimes.json`, from which the
asserted constants A_REL and L2_REL are taken (ten times the largest recorded value, capped at 1e-6).

The tests not marked `gpu` call `nle.sample_grid` and so need the built library, like the rest of the suite: there is no
CPU fallback.
"""
import contextlib
import functools
import json
import math
import os

import numpy as np
import pytest

from conftest import ROOT, load_nle_amd, load_oracle, rel_l2

NR, T, HY, K = 4, 6, 30.0, 8
GRIDS = {  # name -> H, W, sample columns asked for, layers
    "a": dict(H=48, W=256, nc=8, L=3),    # column factors in registers; the recurrence never applies
    "b": dict(H=48, W=250, nc=20, L=3),   # recurrence, the wide Gram, two layers per expand launch; W % 8 = 2, colOff = 10
    "c": dict(H=48, W=253, nc=36, L=3),   # the widest grid the table form takes; colStep = 7
    "d": dict(H=50, W=250, nc=20, L=5),   # as b with five layers: three expand launches of two layers
}
BANDS = ("M-", "M+", "G-", "G+", "U")
THRESHOLD_BANDS = ("M-", "M+", "G-", "G+")
APPLY_WEIGHTS = [2.0, 3.0, 4.0]
ULP32 = 2.0 ** -23            # one fp32 ulp of the output storage, relative
FORM_ENV = ("NLE_SORTED_TABLE", "NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS", "NLE_NO_SORTED_ROWS")

# Ten times the largest figure of profiles/r9_bandwidth_regimes.json (tools/bandwidth_regimes_report.py, all cases on an
# MI355X): the excess of |Y - Y_o| over one fp32 ulp of Y_o relative to max|Y_o[j]|, and the whole-plane relative L2 per
# layer.  Both must stay under CAP = 1e-6, the bar the suite holds fp64-throughout paths to, and no recorded excess may
# pass FINDING = 1e-7 (test_profile_backs_the_asserted_constants checks the record against all three).
CAP = 1e-6
FINDING = 1e-7
A_REL = 2.67e-11
L2_REL = 2.83e-07

CASES = [(g, b, "synthetic") for g in GRIDS for b in BANDS] + [("b", b, "outlier") for b in BANDS]
CASE_IDS = ["%s:%s:%s" % c for c in CASES]
PROFILE = os.path.join(ROOT, "profiles", "r9_bandwidth_regimes.json")


# ------------------------------------------------------------------------------------------------------- the cases
def grid_spec(H, W, nc):
    """the column part of the device's GridSpec, from the oracle's closed form of samplePixels"""
    sel_r, sel_c = load_oracle().sample_grid(H, W, NR, nc)
    return dict(row_step=H // NR, row_off=int(sel_r[0]), n_sel_rows=int(sel_r.size),
                col_step=W // nc, col_off=int(sel_c[0]), n_sel_cols=int(sel_c.size))


def span_of(g, W):
    return max(g["col_off"], W - 1 - g["col_off"]) + g["n_sel_cols"] * g["col_step"]


def predicates(g, W, hx, env=()):
    """Python mirror of sorted_moments_ok, sorted_recurrence and sorted_gsum_ok (csrc/sorted.hip: pure bounds, the m_* < 500 /
    600 terms below) with the exponents they bound, combined as the TableFilter constructor (csrc/sample_space.hip) combines them
    with `env`: the NLE_* measurement variables that force a plain form."""
    cs, nC = float(g["col_step"]), float(g["n_sel_cols"])
    umax = float(max(g["col_off"], W - 1 - g["col_off"]))
    span = umax + nC * cs
    m_e = span * span / (hx * hx)
    m_rho = (2.0 * cs * umax + (2.0 * nC + 1.0) * cs * cs) / (hx * hx)
    m_g = 2.0 * W * W / (hx * hx)
    m_rho_g = (2.0 * cs * W + 2.0 * nC * cs * cs) / (hx * hx)
    table, no_mom, pairs = ("NLE_SORTED_TABLE" in env), ("NLE_SORTED_NO_MOMENTS" in env), ("NLE_GRAM_PAIRS" in env)
    return dict(m_e=m_e, m_rho=m_rho, m_g=m_g, m_rho_g=m_rho_g,
                mom=bool(not table and not no_mom and m_e < 500.0),
                rec=bool(not table and nC > 12 and m_e < 500.0 and m_rho < 500.0),
                gsum=bool(not pairs and W <= 8192 and m_g < 600.0 and m_rho_g < 600.0))   # 8192: sorted_max_width()


def bandwidth(g, W, band):
    if band == "M-":
        return span_of(g, W) / math.sqrt(500.0) * 1.01
    if band == "M+":
        return span_of(g, W) / math.sqrt(500.0) / 1.01
    if band == "G-":
        return W * math.sqrt(2.0 / 600.0) * 1.01
    if band == "G+":
        return W * math.sqrt(2.0 / 600.0) / 1.01
    return W / 30.0


EXPECTED_FORMS = {  # band -> (mom, rec where nC > 12, gsum)
    "M-": (True, True, True), "M+": (False, False, True), "G-": (False, False, True),
    "G+": (False, False, False), "U": (False, False, False),
}


def outlier_image(H, W, sel_mask):
    """a 60 / 120 block checkerboard with +-3 integer noise and about 1 % of the non-sample pixels at 175: those pixels are
    far in level from every sample, so their row sums are small and their Sinkhorn scalings large"""
    rng = np.random.default_rng(29)
    rr, cc = np.mgrid[0:H, 0:W]
    x = np.where(((rr // 8) + (cc // 8)) & 1, 60.0, 120.0) + rng.integers(-3, 4, (H, W))
    out = (rng.random((H, W)) < 0.01) & ~sel_mask
    x[out] = 175.0
    return x


@functools.lru_cache(maxsize=None)
def setup(case):
    """inputs, regions and the oracle's results of one case: computed once, shared by every test, never modified"""
    grid, band, image = case
    oracle = load_oracle()
    H, W, nc, L = (GRIDS[grid][k] for k in ("H", "W", "nc", "L"))
    g = grid_spec(H, W, nc)
    hx = bandwidth(g, W, band)
    sel_r, sel_c = oracle.sample_grid(H, W, NR, nc)
    samples = np.zeros((H, W), dtype=bool)
    samples[np.ix_(sel_r, sel_c)] = True
    x = oracle.synthetic_luminance(H, W) if image == "synthetic" else outlier_image(H, W, samples)
    info = []
    V_o, S_o, inter = oracle.train_filter(x, NR, nc, hx, HY, T, K, return_intermediates=True, info=info)
    Y_o = oracle.apply_layers(V_o, S_o, x, L)
    y_o = oracle.apply_filter(V_o, x, oracle.transform_eigenvalues(S_o, APPLY_WEIGHTS))
    ref = np.concatenate([Y_o, y_o[None]])                      # (L + 1, H, W): the layers, then the weighted apply
    # the row sums that enter inplaceReciprocal in the Sinkhorn loop (src/filter.cpp:238-245), smallest magnitude
    phi, lam = inter["phi"], inter["lam"]
    r, min_sum = np.ones(phi.shape[0]), np.inf
    for _ in range(T):
        v = phi @ (lam * (phi.T @ r))
        min_sum = min(min_sum, float(np.abs(v).min()))
        c, _ = oracle.inplace_reciprocal(v)
        v = phi @ (lam * (phi.T @ c))
        min_sum = min(min_sum, float(np.abs(v).min()))
        r, _ = oracle.inplace_reciprocal(v)
    assert np.array_equal(r, inter["r"]) and np.array_equal(c, inter["c"])    # the loop above is the oracle's
    neigh = np.zeros((H, W), dtype=bool)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                rr, cc = np.nonzero(samples)
                ok = (rr + dr >= 0) & (rr + dr < H) & (cc + dc >= 0) & (cc + dc < W)
                neigh[rr[ok] + dr, cc[ok] + dc] = True
    neigh &= ~samples
    cols = np.arange(W)[None, :].repeat(H, 0)
    regions = {"plane": np.ones((H, W), dtype=bool),
               "tail_cols": cols >= 8 * (W // 8),                               # the last W % 8 columns (none at W = 256)
               "last_slot": (cols >= 8 * (W // 8 - 1)) & (cols < 8 * (W // 8)),  # the last full 8-column slot
               "sample_neighbours": neigh, "samples": samples}
    for a in (x, ref, S_o, *regions.values()):
        a.setflags(write=False)
    return dict(case=case, H=H, W=W, nc=nc, L=L, hx=hx, grid=g, x=x, ref=ref, S_o=S_o, regions=regions,
                pred=predicates(g, W, hx), p=int(samples.sum()), r_Ka=int(lam.size), lam_min=float(lam[-1]),
                kept=[int(i["kept"]) for i in info], min_row_sum=min_sum)


# ------------------------------------------------------------------------------------------------ CPU: the inputs
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cases_sit_where_intended_and_the_oracle_is_well_posed(nle, case):
    grid, band, image = case
    s = setup(case)
    g, W, pr = s["grid"], s["W"], s["pred"]
    assert nle.sample_grid(s["H"], W, NR, s["nc"]) == g                 # the device's grid is the oracle's
    assert g["n_sel_rows"] == NR and g["n_sel_cols"] == s["nc"]
    mom, rec, gsum = EXPECTED_FORMS[band]
    assert (pr["mom"], pr["rec"], pr["gsum"]) == (mom, rec and s["nc"] > 12, gsum), pr
    if band in ("M-", "M+"):
        assert abs(pr["m_e"] / 500.0 - 1.0) < 0.03 and (pr["m_e"] < 500.0) == (band == "M-"), pr
        assert pr["m_rho"] < pr["m_e"]                                   # m_rho never binds first
    if band in ("G-", "G+"):
        assert abs(pr["m_g"] / 600.0 - 1.0) < 0.03 and (pr["m_g"] < 600.0) == (band == "G-"), pr
        assert pr["m_rho_g"] < 600.0 and pr["m_e"] > 500.0, pr           # the Gram's own bound decides, moments are off
    if band == "U":                                                      # the distance table reaches 0 inside one row
        assert math.exp(-float(W - 1) ** 2 / s["hx"] ** 2) == 0.0 and abs(W / s["hx"] - 30.0) < 1e-12
    # forcing the plain forms changes the mirrored choice exactly where a reformulation is on
    forced = predicates(g, W, s["hx"], env=("NLE_SORTED_TABLE", "NLE_GRAM_PAIRS"))
    assert not (forced["mom"] or forced["rec"] or forced["gsum"])
    assert np.all(s["x"] == np.rint(s["x"])) and s["x"].min() >= 0 and s["x"].max() <= 255   # auto mode takes the tables
    assert s["r_Ka"] == s["p"] == NR * s["nc"], (s["r_Ka"], s["p"])      # r == p
    assert s["lam_min"] > 1e-3, s["lam_min"]
    assert s["S_o"].size == K and s["kept"][0] == s["p"], s["kept"]      # K' == K
    if image == "outlier":
        assert (s["x"] == 175.0).sum() >= 0.005 * s["x"].size and not np.any(s["x"][s["regions"]["samples"]] == 175.0)
        assert s["min_row_sum"] >= 1e-7, s["min_row_sum"]                # 1000 x the eps = 1e-10 cut: no zeroing is borderline
    assert s["regions"]["sample_neighbours"].sum() == 8 * s["p"]
    assert s["regions"]["tail_cols"].sum() == s["H"] * (W % 8) and s["regions"]["last_slot"].sum() == 8 * s["H"]


def test_m_rho_cannot_bind_before_m_e():
    """sorted_recurrence checks m_rho < 500 too; (umax + nC cs)^2 >= 2 cs umax + (2 nC + 1) cs^2 for nC >= 2, so m_e binds
    first on every grid the recurrence is used on"""
    for W in (37, 250, 253, 256, 700, 4096):
        for nc in range(2, 37):
            if nc > W:
                continue
            g = grid_spec(48, W, nc)
            pr = predicates(g, W, 10.0)
            assert pr["m_rho"] <= pr["m_e"], (W, nc, pr)


def test_profile_backs_the_asserted_constants():
    """A_REL and L2_REL are ten times the largest figures recorded on an MI355X and under the 1e-6 cap, and no recorded
    excess is above 1e-7"""
    with open(PROFILE) as fh:
        prof = json.load(fh)
    assert sorted(prof["cases"]) == sorted(CASE_IDS)
    for cid, c in prof["cases"].items():
        assert set(c) >= {"predicates", "eig_err", "excess", "rel_l2", "forced_plain"}, cid
        assert set(c["excess"]) == {"plane", "tail_cols", "last_slot", "sample_neighbours", "samples"}, cid
    mx_a = max(max(max(v) for v in c["excess"].values()) for c in prof["cases"].values())
    mx_l2 = max(max(c["rel_l2"]) for c in prof["cases"].values())
    assert mx_a == prof["max_excess"] and mx_l2 == prof["max_rel_l2"]
    assert mx_a <= FINDING, mx_a                                          # anything above is a finding, not a tolerance
    assert 10.0 * mx_a <= A_REL <= 10.5 * mx_a and A_REL <= CAP, (mx_a, A_REL)
    assert 10.0 * mx_l2 <= L2_REL <= 10.5 * mx_l2 and L2_REL <= CAP, (mx_l2, L2_REL)


# ------------------------------------------------------------------------------------------------ GPU: the record
@contextlib.contextmanager
def forms(*names):
    """run with exactly these measurement variables set (and none of the others that select a kernel form)"""
    saved = {k: os.environ.pop(k) for k in FORM_ENV if k in os.environ}
    os.environ.update({k: "1" for k in names})
    try:
        yield
    finally:
        for k in names:
            del os.environ[k]
        os.environ.update(saved)


def run_device(s, *env):
    """one train + apply_layers + apply on a fresh Context; float32 planes as the device wrote them"""
    nle = load_nle_amd()
    x32 = s["x"].astype(np.float32)
    with forms(*env):
        c = nle.Context(0)
        f = nle.NLEFilter(c).train_filter(x32, NR, s["nc"], s["hx"], HY, T, K)
        d, ev = f.diag(), f.eigvals.copy()
        Y = f.apply_layers(x32, s["L"]).cpu().numpy().reshape(s["L"], s["H"], s["W"])
        y = f.apply(x32, nle.transform_eigenvalues(ev, APPLY_WEIGHTS)).cpu().numpy().reshape(1, s["H"], s["W"])
        f.close()
        c.close()
    return dict(diag=d, ev=ev, Y=np.concatenate([Y, y]))


def bitwise(a, b):
    return a["ev"].tobytes() == b["ev"].tobytes() and a["Y"].tobytes() == b["Y"].tobytes()


def excess(Y, ref, scale, mask):
    """per plane j: max over the pixels of `mask` of (|Y - ref| - 2^-23 |ref|) / max|scale[j]|, floored at 0"""
    out = []
    for j in range(ref.shape[0]):
        d = np.abs(Y[j].astype(np.float64)[mask] - ref[j][mask]) - ULP32 * np.abs(ref[j][mask])
        if not np.all(np.isfinite(d)):
            out.append(math.inf)                       # a NaN must not vanish in a max()
        else:
            out.append(max(0.0, float(d.max())) / float(np.abs(scale[j]).max()) if d.size else 0.0)
    return out


def against(run, base, ref):
    """a forced-form run against the default run: bitwise or not, the cross-form figures of
    test_level_sorted_rows_..., and the elementwise excess (over one ulp of the default, in units of max|Y_o[j]|)"""
    Yb = base["Y"].astype(np.float64)
    return dict(bitwise=bitwise(run, base), eig=rel_l2(run["ev"], base["ev"]),
                rel_l2=[rel_l2(run["Y"][j], base["Y"][j]) for j in range(Yb.shape[0])],
                excess=excess(run["Y"], Yb, ref, np.ones(Yb.shape[1:], dtype=bool)))


_RECORDS = {}


def record(case):
    """the figures of one case, computed once.  A failure is kept too and raised again for every later test of the case:
    device code that has failed once is not started a second time."""
    if case not in _RECORDS:
        try:
            _RECORDS[case] = _record(case)
        except (Exception, pytest.fail.Exception) as e:   # an error from the device, or a per-test time limit (pytest.fail)
            _RECORDS[case] = e
            raise
    if isinstance(_RECORDS[case], BaseException):
        raise RuntimeError("the device runs of %s failed earlier: %r" % (case, _RECORDS[case]))
    return _RECORDS[case]


def _record(case):
    """every figure of one case, from the device runs it needs: the default run against the oracle, the forced plain forms
    against the default run, the moment predicate alone (M-, M+), a second default run (threshold cases)"""
    s = setup(case)
    band, ref = case[1], s["ref"]
    base = run_device(s)
    rec = dict(W_over_hx=s["W"] / s["hx"], predicates=s["pred"], diag=base["diag"],
               eig_err=rel_l2(base["ev"], s["S_o"]) if base["ev"].size == s["S_o"].size else math.inf,   # K' differs
               excess={k: excess(base["Y"], ref, ref, m) for k, m in s["regions"].items()},
               rel_l2=[rel_l2(base["Y"][j], ref[j]) for j in range(ref.shape[0])],
               forced_plain=against(run_device(s, "NLE_SORTED_TABLE", "NLE_GRAM_PAIRS"), base, ref))
    if band in ("M-", "M+"):
        rec["no_moments"] = against(run_device(s, "NLE_SORTED_NO_MOMENTS"), base, ref)
    if band in THRESHOLD_BANDS:
        rec["repeat_bitwise"] = bitwise(run_device(s), base)
    return rec


def planes(s):
    return ["layer %d" % j for j in range(s["L"])] + ["apply %s" % APPLY_WEIGHTS]


# ------------------------------------------------------------------------------------------- GPU: device vs oracle
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_table_form_is_taken_and_ranks_and_eigenvalues_are_the_oracles(nle, case):
    s, rec = setup(case), record(case)
    d = rec["diag"]
    assert d["formulation"] == nle.MODE_PHI_FREE, d
    assert (d["p"], d["r_Ka"], d["r_Wa"], d["r_Q"], d["K"]) == (s["p"], *s["kept"], s["S_o"].size), (d, s["kept"])
    print(case, "eigenvalues rel L2 %.2e" % rec["eig_err"])
    assert rec["eig_err"] < 1e-9, rec["eig_err"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_pixel_of_every_layer_is_within_one_ulp_of_the_oracle(case):
    s, rec = setup(case), record(case)
    print(case, "excess over one fp32 ulp / max|Y_o[j]|:", ["%.2e" % e for e in rec["excess"]["plane"]],
          " rel L2:", ["%.2e" % e for e in rec["rel_l2"]])
    for name, e, l2 in zip(planes(s), rec["excess"]["plane"], rec["rel_l2"]):
        assert e <= A_REL, "%s: a pixel is %.3e max|Y_o| beyond one fp32 ulp of the oracle (bound %.1e)" % (name, e, A_REL)
        assert l2 <= L2_REL, "%s: whole-plane relative L2 %.3e (bound %.1e)" % (name, l2, L2_REL)


REGION_CASES = [(c, r) for c in CASES for r in ("tail_cols", "last_slot", "sample_neighbours", "samples")
                if not (r == "tail_cols" and GRIDS[c[0]]["W"] % 8 == 0)]      # W = 256 has no partial slot


@pytest.mark.gpu
@pytest.mark.parametrize("case,region", REGION_CASES, ids=["%s:%s:%s-%s" % (*c, r) for c, r in REGION_CASES])
def test_named_pixels_are_within_one_ulp_of_the_oracle(case, region):
    """the pixels a whole-plane norm hides: the last W % 8 columns and the last full 8-column slot of every row, the eight
    neighbours of every sample pixel, and the sample pixels (written by scatter_samples, not by the expand kernel)"""
    s, rec = setup(case), record(case)
    assert s["regions"][region].any()
    for name, e in zip(planes(s), rec["excess"][region]):
        assert e <= A_REL, "%s, %s: %.3e max|Y_o| beyond one fp32 ulp of the oracle (bound %.1e)" % (region, name, e, A_REL)


# -------------------------------------------------------------------------------- GPU: which form ran, by bitwise evidence
def _agrees_across_forms(s, cmp, what):
    assert cmp["eig"] < 1e-10, (what, cmp["eig"])                       # the standing cross-form bars
    for name, l2, e in zip(planes(s), cmp["rel_l2"], cmp["excess"]):
        assert l2 < 1e-7, (what, name, l2)
        assert e <= A_REL, "%s, %s: %.3e max|Y_o| beyond one fp32 ulp of the default run" % (what, name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forcing_the_plain_forms_changes_bits_exactly_where_a_predicate_is_on(case):
    s, rec = setup(case), record(case)
    pr, cmp = s["pred"], rec["forced_plain"]
    print(case, "forced plain forms: bitwise", cmp["bitwise"], "eig %.2e" % cmp["eig"], ["%.2e" % e for e in cmp["rel_l2"]])
    if pr["mom"] or pr["rec"] or pr["gsum"]:
        assert not cmp["bitwise"], "a reformulation should be on here, yet the plain forms give the same bits"
        _agrees_across_forms(s, cmp, "forced plain forms")
    else:
        assert cmp["bitwise"], "every form should already be plain here, yet forcing them changed the result"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[1] in ("M-", "M+")],
                         ids=[i for c, i in zip(CASES, CASE_IDS) if c[1] in ("M-", "M+")])
def test_the_moment_predicate_flips_between_the_threshold_pair(case):
    """NLE_SORTED_NO_MOMENTS alone: 2 % inside the bound the moment form is on (other bits, same result), 2 % outside the
    predicate has already turned it off and the variable is a bitwise no-op.  With 8 sample columns nothing else differs."""
    s, rec = setup(case), record(case)
    cmp = rec["no_moments"]
    if case[1] == "M-":
        assert s["pred"]["mom"] and not cmp["bitwise"]
        _agrees_across_forms(s, cmp, "without moments")
    else:
        assert not s["pred"]["mom"] and cmp["bitwise"], "the moment form ran beyond its bound"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[1] in THRESHOLD_BANDS],
                         ids=[i for c, i in zip(CASES, CASE_IDS) if c[1] in THRESHOLD_BANDS])
def test_threshold_cases_are_bitwise_reproducible(case):
    assert record(case)["repeat_bitwise"]
