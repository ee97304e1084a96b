"""The level-sorted rows (csrc/sorted.hip, csrc/sorted_rows.h, csrc/sorted_planes.hip) at their widest rows and longest chunks.

`k_sort_rows` cuts every image row into at most 512 chunks of one level each; the chunk length CH is the smallest with
sum_x ceil(tot[x] / CH) <= 512, and a chunk's slot holds CHP = CH rounded up to four entries, at most 32 at
`sorted_max_width()` = 8192 columns (eight blocks of four indices, `kMaxBlocks`).  The other tests stay at the short end of
that layout: CHP <= 24, no level with all 512 chunks, no row without a non-sample pixel.  The planes here are built to reach
the far end, H = 8 rows of named kinds with one sample row (nr = 1: row 3):

  one-heavy   255 levels of one pixel each at random columns, every other pixel on one level: the only kind of row that
              reaches CH = 29 .. 31 (CHP = 32: the 7th and 8th index block of `load_chunk_idx`)
  flat        one level: m = 512 chunks of it at W = 4096 and 8192 (j runs through its whole 9-bit field, nine tree steps)
  two         0 / 255 alternating: the two extreme level tiles
  noise       uniform over the 256 levels (CHP 12 .. 24)
  ramp        floor(256 c / W)
  smooth      a sine with +-12 noise

in the order one-heavy, flat, two, noise, one-heavy, ramp, smooth, noise, so that consecutive rows differ in slot size.  One
variant puts a one-heavy row in the sample row with three of its singleton levels ON sample columns: those levels are in the
level plane and have no pixel in the sorted row (tot[x] = 0).  Widths sit on either side of the four / two layers per launch
switch of `k_sorted_expand` (4096 / 4097), at the widest CH = 29 (7452), at the last odd width (8191), at the limit (8192)
and one past it (8193: the train must fall back to the unsorted kernels).  The narrow cases (W = 12, 16, 36 with nC = W,
nr = 2) have sample rows in which EVERY pixel is a sample: wn = 0, no chunk, every thread idle.

hx = W / 8 (narrow: 4, 4 and 3.5) lies inside all three bandwidth predicates (test_sorted_dispatch.py), so the moment pass,
the recurrence beyond 12 columns and the index-sum Gram run by default; hy = 100, T = 8, K = min(8, nC), L = 3.  The
tests not marked `gpu` state what the inputs must reach (a numpy mirror of the CH rule) and that the oracle is well posed
on them (test_bandwidth_regimes.py's conditions), and print the CH / CHP / m table with the kernel forms of each case.

On the device every case is computed once (`runs`) and held to
  the CPU oracle            layers 1e-4 relative L2, eigenvalues 1e-8, every pixel |Y - Y_o| <= 2^-23 |Y_o| + CAP max|Y_o[j]|
                            (CAP = 1e-6, test_bandwidth_regimes.py), again on the regions a plane norm hides
  the unsorted kernels      NLE_NO_SORTED_ROWS, image order and LDS atomics: eigenvalues 1e-9, layers 1e-6, the CAP form
  the forced forms          NLE_SORTED_TABLE; NLE_SORTED_NO_MOMENTS + NLE_GRAM_PAIRS: eigenvalues 1e-10, layers 1e-7
  itself                    a second default run, bit for bit
and, where listed, apply_layers on either side of the layer switch, V rebuilt from the sorted rows (`k_rows_from_sorted`)
against the V of the unsorted filter, `apply_planes` against the single calls bit for bit, apply with and without
training's reduce half bit for bit.  One tall case (H = CUs + 9 under NLE_SORTED_WGS_PER_CU=1) gives some workgroups a
second row with another slot size than the first.  Figures of an MI355X run: profiles/r16_wide_rows.txt.
"""
import functools

import numpy as np
import pytest

from conftest import load_oracle, rel_l2
from test_bandwidth_regimes import CAP, FINDING, excess, predicates
from test_expand_edges import n_cus

H, HY, T, L = 8, 100.0, 8, 3
SEED = 16
KT = 512                                  # kSortedThreads: chunks per row
ORDER = ("one-heavy", "flat", "two", "noise", "one-heavy", "ramp", "smooth", "noise")
VARIANT_ORDER = ("one-heavy", "flat", "two", "one-heavy", "one-heavy", "ramp", "smooth", "noise")
NARROW_ORDER = ("flat", "noise", "two", "noise", "ramp", "noise", "smooth", "noise")     # sample rows 1 and 5: noise
TALL_ORDER = ("one-heavy", "flat", "two", "noise", "smooth", "ramp", "noise")
NARROW_HX = {12: 4.0, 16: 4.0, 36: 3.5}     # inside the three predicates too, and lambda_min(K_A) > 1e-3 on the oracle
FORM_ENV = ("NLE_SORTED_TABLE", "NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS", "NLE_NO_SORTED_ROWS", "NLE_ALL_LEVEL_TILES",
            "NLE_SORTED_WGS_PER_CU")
UNSORTED = ("NLE_NO_SORTED_ROWS",)
TABLE = ("NLE_SORTED_TABLE",)
FORCED = ("NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS")

# name -> W, sample columns asked for, sample rows, which plane
CASES = {
    "4096:10": dict(W=4096, nc=10, nr=1, plane="wide"),
    "4097:10": dict(W=4097, nc=10, nr=1, plane="wide"),
    "4097:13": dict(W=4097, nc=13, nr=1, plane="wide"),
    "7452:13": dict(W=7452, nc=13, nr=1, plane="wide"),
    "8191:36": dict(W=8191, nc=36, nr=1, plane="wide"),
    "8192:10": dict(W=8192, nc=10, nr=1, plane="wide"),
    "8192:13": dict(W=8192, nc=13, nr=1, plane="wide"),
    "8192:36": dict(W=8192, nc=36, nr=1, plane="wide"),
    "8192:10:heavy-sample-row": dict(W=8192, nc=10, nr=1, plane="variant"),
    "8193:10": dict(W=8193, nc=10, nr=1, plane="wide"),
    "narrow:12": dict(W=12, nc=12, nr=2, plane="narrow"),
    "narrow:16": dict(W=16, nc=16, nr=2, plane="narrow"),
    "narrow:36": dict(W=36, nc=36, nr=2, plane="narrow"),
}
ALL = list(CASES)
SORTED = [c for c in ALL if CASES[c]["W"] <= 8192]                  # 8193 falls back: its default run IS the unsorted one
LAYER_CASES = {"4096:10": (1, 4, 5), "4097:10": (1, 4, 5), "8192:13": (1, 2, 3)}   # four per launch | two | two
REBUILD_CASES = ["8192:10", "8192:10:heavy-sample-row", "narrow:12", "narrow:16", "narrow:36"]
PLANES_CASES = {"8192:10": 5, "8192:13": 3}                           # four planes per launch + one | two + one
REUSE_CASE = "8192:10"
APPLY_WEIGHTS = [2.0, 3.0, 4.0]


# ------------------------------------------------------------------------------------------------------- the planes
def make_row(kind, W, rng, pinned=None):
    """one row of a named kind; `pinned`: columns that must hold singleton levels of a one-heavy row"""
    c = np.arange(W)
    if kind == "one-heavy":
        heavy = int(rng.integers(0, 256))
        levels = rng.permutation(np.array([v for v in range(256) if v != heavy]))
        if pinned is None:
            cols = rng.choice(W, 255, replace=False)
        else:
            rest = rng.choice(np.setdiff1d(c, pinned), 255 - len(pinned), replace=False)
            cols = np.concatenate([np.asarray(pinned), rest])
        row = np.full(W, heavy)
        row[cols] = levels
        return row.astype(np.float64)
    if kind == "flat":
        return np.full(W, float(rng.integers(0, 256)))
    if kind == "two":
        return (c & 1) * 255.0
    if kind == "noise":
        return rng.integers(0, 256, W).astype(np.float64)
    if kind == "ramp":
        return np.floor(256.0 * c / W)
    assert kind == "smooth"
    return np.clip(np.rint(128.0 + 90.0 * np.sin(2.0 * np.pi * c * 3.0 / W) + rng.integers(-12, 13, W)), 0.0, 255.0)


def make_plane(order, W, rows, sel_r, sel_c, pin_sample_row=False):
    """`rows` rows cycling through `order`; with pin_sample_row the one-heavy row that is the sample row gets singleton
    levels on the first, the middle and the last sample column"""
    rng = np.random.default_rng(SEED)
    kinds = tuple(order[r % len(order)] for r in range(rows))
    x = np.empty((rows, W))
    for r, kind in enumerate(kinds):
        pinned = None
        if pin_sample_row and r in sel_r:
            assert kind == "one-heavy"
            pinned = sel_c[[0, sel_c.size // 2, sel_c.size - 1]]
        x[r] = make_row(kind, W, rng, pinned)
    assert np.array_equal(x, np.rint(x)) and x.min() >= 0.0 and x.max() <= 255.0     # auto mode takes the tables
    return x, kinds


def chunking(row, is_sample):
    """numpy mirror of k_sort_rows' cut of one image row: the level counts without the sample pixels, the smallest CH with
    sum_x ceil(tot[x] / CH) <= 512, the slot size and the largest number of chunks of one level"""
    tot = np.bincount(row[~is_sample].astype(np.int64), minlength=256)
    wn = int(tot.sum())
    CH = 1
    while int((-(-tot // CH)).sum()) > KT:
        CH += 1
    m = -(-tot // CH)
    return dict(wn=wn, tot=tot, CH=CH, CHP=(CH + 3) & ~3, max_m=int(m.max()), chunks=int(m.sum()), levels=int((tot > 0).sum()))


@functools.lru_cache(maxsize=None)
def setup(case):
    """inputs, regions, the chunk table and the oracle's results of one case: computed once, shared, never modified"""
    oracle = load_oracle()
    W, nc, nr, which = (CASES[case][k] for k in ("W", "nc", "nr", "plane"))
    hx = NARROW_HX[W] if which == "narrow" else W / 8.0
    K = min(8, nc)
    sel_r, sel_c = oracle.sample_grid(H, W, nr, nc)
    order = {"wide": ORDER, "variant": VARIANT_ORDER, "narrow": NARROW_ORDER}[which]
    x, kinds = make_plane(order, W, H, sel_r, sel_c, pin_sample_row=which == "variant")
    samples = np.zeros((H, W), dtype=bool)
    samples[np.ix_(sel_r, sel_c)] = True
    g = dict(row_step=H // nr, row_off=int(sel_r[0]), n_sel_rows=int(sel_r.size),
             col_step=W // nc, col_off=int(sel_c[0]), n_sel_cols=int(sel_c.size))
    info = []
    V_o, S_o, inter = oracle.train_filter(x, nr, nc, hx, HY, T, K, return_intermediates=True, info=info)
    neigh = np.zeros((H, W), dtype=bool)
    rr, cc = np.nonzero(samples)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                ok = (rr + dr >= 0) & (rr + dr < H) & (cc + dc >= 0) & (cc + dc < W)
                neigh[rr[ok] + dr, cc[ok] + dc] = True
    neigh &= ~samples
    cols = np.arange(W)[None, :].repeat(H, 0)
    regions = {"plane": np.ones((H, W), dtype=bool),
               "tail_cols": cols >= 8 * (W // 8),                               # the last W % 8 columns
               "last_slot": (cols >= 8 * (W // 8 - 1)) & (cols < 8 * (W // 8)),  # the last full 8-column slot
               "samples": samples, "sample_neighbours": neigh}
    for kind in sorted(set(kinds)):
        regions["rows:" + kind] = np.array([k == kind for k in kinds])[:, None].repeat(W, 1)
    for a in (x, V_o, S_o, *regions.values()):
        a.setflags(write=False)
    return dict(case=case, W=W, nc=nc, nr=nr, hx=hx, K=K, x=x, kinds=kinds, grid=g, sel_r=sel_r, sel_c=sel_c, regions=regions,
                chunks=[chunking(x[r], samples[r]) for r in range(H)], pred=predicates(g, W, hx),
                V_o=V_o, S_o=S_o, p=int(samples.sum()), lam=inter["lam"], kept=[int(i["kept"]) for i in info])


@functools.lru_cache(maxsize=None)
def oracle_layers(case, n_layers):
    """the oracle's layers of the training plane, (n_layers, H, W)"""
    s = setup(case)
    Y = load_oracle().apply_layers(s["V_o"], s["S_o"], s["x"], n_layers)
    Y.setflags(write=False)
    return Y


def forms_of(s):
    """which form of the pass, the column factors and the Gram runs (test_bandwidth_regimes.predicates)"""
    if s["W"] > 8192:
        return "unsorted"
    pr = s["pred"]
    return "pass %s, expand %s, Gram %s" % ("mom" if pr["mom"] else "rec" if pr["rec"] else "table",
                                            "rec" if pr["rec"] else "table", "gsum" if pr["gsum"] else "pairs")


# ------------------------------------------------------------------------------------------------ CPU: the inputs
def rows_of(s, kind):
    return [r for r in range(H) if s["kinds"][r] == kind]


@pytest.mark.parametrize("case", ALL)
def test_the_rows_reach_the_chunking_they_are_there_for(case):
    s = setup(case)
    W, ch = s["W"], s["chunks"]
    print("\n%s  hx %.4g  p %d  forms: %s" % (case, s["hx"], s["p"], forms_of(s)))
    for r in range(H):
        c = ch[r]
        print("  row %d %-9s %s wn %4d  levels %3d  CH %2d  CHP %2d  chunks %3d  max m %3d"
              % (r, s["kinds"][r], "S" if r in s["sel_r"] else " ", c["wn"], c["levels"], c["CH"], c["CHP"], c["chunks"], c["max_m"]))
    for c in ch:                                                     # the layout's own limits
        assert c["chunks"] <= KT and c["CH"] <= 32 and c["max_m"] <= KT
        assert c["CHP"] <= 4 * ((((W + 255) // 256) + 3) // 4)           # sorted_chp_max(W)
    assert s["grid"]["n_sel_rows"] == s["nr"] and s["grid"]["n_sel_cols"] == s["nc"]
    if CASES[case]["plane"] == "narrow":
        assert s["grid"]["col_step"] == 1 and s["sel_c"].size == W       # every column is a sample column
        for r in s["sel_r"]:
            assert ch[r]["wn"] == 0 and ch[r]["chunks"] == 0 and ch[r]["CH"] == 1
        return
    heavy = [ch[r] for r in rows_of(s, "one-heavy")]
    assert len(heavy) >= 2
    want = {4096: (15, 16), 4097: (15, 16), 7452: (29, 32), 8191: (31, 32), 8192: (31, 32), 8193: (31, 32)}[W]
    for c in heavy:
        assert (c["CH"], c["CHP"]) == want, (c["CH"], c["CHP"], want)
    if W >= 7452:
        assert all(c["CHP"] == 32 for c in heavy)                       # the 7th and 8th index block
    flat = ch[rows_of(s, "flat")[0]]
    if W in (4096, 8192):
        assert flat["max_m"] == KT and flat["levels"] == 1 and flat["CH"] == W // KT
    for r in rows_of(s, "noise"):
        assert 12 <= ch[r]["CHP"] <= 24, ch[r]["CHP"]
    assert len({c["CHP"] for c in ch}) >= 2                             # rows of one image differ in slot size
    if CASES[case]["plane"] == "variant":
        (r,) = s["sel_r"]
        assert s["kinds"][r] == "one-heavy"
        on_sample = [int(v) for v in s["x"][r, s["sel_c"]] if (s["x"][r] == v).sum() == 1]
        assert len(on_sample) >= 3, on_sample
        for v in on_sample:                                             # in the level plane, not in the sorted row
            assert ch[r]["tot"][v] == 0 and (s["x"][r] == v).any()
        assert ch[r]["levels"] == 256 - len(on_sample) and ch[r]["CHP"] == 32
    else:
        assert s["kinds"][int(s["sel_r"][0])] == "noise" and int(s["sel_r"][0]) == 3


@pytest.mark.parametrize("case", ALL)
def test_the_oracle_is_well_posed(case):
    s = setup(case)
    pr, p, K = s["pred"], s["p"], s["K"]
    top = float(s["S_o"][0])
    layer_sets = sorted({L, *LAYER_CASES.get(case, ())})
    norms = {n: [float(np.linalg.norm(y)) for y in oracle_layers(case, n)] for n in layer_sets}
    print("\n%s  lambda_min(K_A) %.3e  kept %s of %d  K %d  top eigenvalue %.6f  layer norms %s"
          % (case, s["lam"][-1], s["kept"], p, s["S_o"].size, top, {n: ["%.3g" % v for v in norms[n]] for n in norms}))
    assert p == s["nr"] * s["nc"] and s["lam"].size == p
    assert s["lam"][-1] > 1e-3, s["lam"][-1]
    assert s["kept"] == [p, p, p] and s["S_o"].size == K, (s["kept"], s["S_o"].size)
    assert 0.99 <= top <= 1.01, top
    for n, v in norms.items():
        assert min(v) > 1.0, (n, v)
    # inside all three predicates: the moment pass, the recurrence beyond 12 columns, the Gram on index sums
    assert pr["m_e"] < 500.0 and pr["m_rho"] < 500.0 and pr["m_g"] < 600.0 and pr["m_rho_g"] < 600.0, pr
    assert pr["mom"] and pr["rec"] == (s["nc"] > 12) and pr["gsum"] == (s["W"] <= 8192), pr


# ------------------------------------------------------------------------------------------------ GPU: the runs
def _env(monkeypatch, names, value="1"):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k in names:
        monkeypatch.setenv(k, value)


def _train(nle, ctx, monkeypatch, s, x32, env=()):
    _env(monkeypatch, env)
    try:
        return nle.NLEFilter(ctx).train_filter(x32, s["nr"], s["nc"], s["hx"], HY, T, s["K"])
    finally:
        _env(monkeypatch, ())


def _layers(f, x32, n_layers, shape):
    return f.apply_layers(x32, n_layers).cpu().numpy().reshape(n_layers, *shape)


def _run(nle, ctx, monkeypatch, s, env=(), extras=None):
    """one train + apply_layers; `extras(f)` runs on the open filter"""
    x32 = s["x"].astype(np.float32)
    f = _train(nle, ctx, monkeypatch, s, x32, env)
    try:
        out = dict(diag=f.diag(), ev=f.eigvals.copy(), Y=_layers(f, x32, L, x32.shape))
        if extras is not None:
            out.update(extras(f, x32))
        return out
    finally:
        f.close()


def make_planes(x, count):
    """the training plane, a rolled copy and a non-integer plane, in turn"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for m in range(count):
        if m % 3 == 0:
            p = np.roll(x, (m // 3, 17 * m), (0, 1)) if m else x
        elif m % 3 == 1:
            p = np.roll(x, (1 + m // 3, 1001 + m), (0, 1))
        else:
            p = x * 0.37 + rng.standard_normal(x.shape)
        out.append(p.astype(np.float32))
    assert np.array_equal(out[0], x.astype(np.float32)) and not np.array_equal(out[2], np.rint(out[2]))
    return np.stack(out)


def _extras(nle, ctx, case, s):
    def extras(f, x32):
        out = {}
        if case in LAYER_CASES:
            out["layers"] = {n: _layers(f, x32, n, x32.shape) for n in LAYER_CASES[case]}
        if case in REBUILD_CASES:
            out["V"] = f.eigvecs().cpu().numpy()[:, :f.info()["K"]]
        if case in PLANES_CASES:
            P = PLANES_CASES[case]
            planes = make_planes(s["x"], P)
            rng = np.random.default_rng(SEED + 2)
            resp = [nle.transform_eigenvalues(f.eigvals, APPLY_WEIGHTS)] + [rng.uniform(0.1, 2.0, f.info()["K"]) for _ in range(P - 1)]
            ctx.profile(1)
            try:
                batch = {kind: f.apply_planes(planes, resp, out_kind=kind).cpu().numpy() for kind in (0, 1)}
                launches = ctx.kernel_stats()["apply_reduce"][0]
            finally:
                ctx.profile(0)
            single = {0: np.stack([f.apply(planes[m], resp[m]).cpu().numpy() for m in range(P)]),
                      1: np.stack([f.apply_rounded8(planes[m], resp[m]).cpu().numpy() for m in range(P)])}
            out["planes"] = dict(batch=batch, single=single, launches=launches, P=P)
        if case == REUSE_CASE:
            fs = nle.transform_eigenvalues(f.eigvals, APPLY_WEIGHTS)
            out["apply"] = f.apply(x32, fs).cpu().numpy()
            ctx.set_train_reduce(False)
            try:                                                        # the switch at apply time alone, on this filter
                out["apply_off_at_apply"] = f.apply(x32, fs).cpu().numpy()
            finally:
                ctx.set_train_reduce(True)
        return out
    return extras


def _unsorted_extras(case):
    def extras(f, x32):
        return {"V": f.eigvecs().cpu().numpy()[:, :f.info()["K"]]} if case in REBUILD_CASES else {}
    return extras


_RUNS = {}


def runs(nle, ctx, monkeypatch, case):
    """every device run of one case, made once; a failure is kept and raised again (device code that failed once is not
    started a second time)"""
    if case not in _RUNS:
        try:
            s = setup(case)
            out = {"default": _run(nle, ctx, monkeypatch, s, extras=_extras(nle, ctx, case, s))}
            if case in SORTED:
                out["again"] = _run(nle, ctx, monkeypatch, s)
                out["unsorted"] = _run(nle, ctx, monkeypatch, s, UNSORTED, extras=_unsorted_extras(case))
                out["table"] = _run(nle, ctx, monkeypatch, s, TABLE)
                out["forced"] = _run(nle, ctx, monkeypatch, s, FORCED)
            if case == REUSE_CASE:
                ctx.set_train_reduce(False)
                try:                                                    # trained without the reuse, applied without it
                    fs_of = lambda f, x32: {"apply": f.apply(x32, nle.transform_eigenvalues(f.eigvals, APPLY_WEIGHTS)).cpu().numpy()}
                    out["reuse_off"] = _run(nle, ctx, monkeypatch, s, extras=fs_of)
                finally:
                    ctx.set_train_reduce(True)
            _RUNS[case] = out
        except (Exception, pytest.fail.Exception) as e:
            _RUNS[case] = e
            raise
    if isinstance(_RUNS[case], BaseException):
        raise RuntimeError("the device runs of %s failed earlier: %r" % (case, _RUNS[case]))
    return _RUNS[case]


def _fmt(v):
    return " ".join("%.2e" % e for e in v)


def _note_findings(case, what, figures):
    worst = max(figures)
    if worst > FINDING:
        print("wide_rows FINDING %s %s: per-pixel excess %.3e above %.0e (below CAP = %.0e it does not fail)" % (case, what, worst, FINDING, CAP))


# ------------------------------------------------------------------------------------------- GPU: device vs oracle
@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_layers_and_eigenvalues_are_the_oracles(nle, ctx, monkeypatch, case):
    s, r = setup(case), runs(nle, ctx, monkeypatch, case)["default"]
    d, Y_o = r["diag"], oracle_layers(case, L)
    assert d["formulation"] == nle.MODE_PHI_FREE, d                     # also at 8193: the unsorted kernels take it
    assert (d["p"], d["r_Ka"], d["r_Wa"], d["r_Q"], d["K"]) == (s["p"], *s["kept"], s["S_o"].size), (d, s["kept"])
    e_eig = rel_l2(r["ev"], s["S_o"])
    l2 = [rel_l2(r["Y"][j], Y_o[j]) for j in range(L)]
    ex = excess(r["Y"], Y_o, Y_o, s["regions"]["plane"])
    print("\nwide_rows %s [%s] against the oracle: eigenvalues %.2e  layers rel L2 %s  largest per-pixel excess %s"
          % (case, forms_of(s), e_eig, _fmt(l2), _fmt(ex)))
    _note_findings(case, "against the oracle", ex)
    assert np.isfinite(r["Y"]).all()
    assert e_eig < 1e-8, e_eig
    assert max(l2) < 1e-4, l2
    for j, e in enumerate(ex):
        assert e <= CAP, "layer %d: a pixel is %.3e max|Y_o| beyond one fp32 ulp of the oracle (bound %.1e)" % (j, e, CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_the_pixels_a_plane_norm_hides_are_the_oracles(nle, ctx, monkeypatch, case):
    """the last W % 8 columns, the last full 8-column slot, the sample pixels (k_scatter_samples), their neighbours, and the
    rows of each kind on their own"""
    s, r = setup(case), runs(nle, ctx, monkeypatch, case)["default"]
    Y_o = oracle_layers(case, L)
    for name, mask in s["regions"].items():
        if name == "plane":
            continue
        assert mask.any() or (name == "tail_cols" and s["W"] % 8 == 0), name
        ex = excess(r["Y"], Y_o, Y_o, mask)
        print("wide_rows %s region %-18s %6d pixels: per-pixel excess %s" % (case, name, int(mask.sum()), _fmt(ex)))
        for j, e in enumerate(ex):
            assert e <= CAP, "%s, layer %d: %.3e max|Y_o| beyond one fp32 ulp of the oracle (bound %.1e)" % (name, j, e, CAP)


# ------------------------------------------------------------------------------------- GPU: the other kernel forms
@pytest.mark.gpu
@pytest.mark.parametrize("case", SORTED)
def test_sorted_rows_agree_with_the_unsorted_kernels(nle, ctx, monkeypatch, case):
    rs = runs(nle, ctx, monkeypatch, case)
    base, uns = rs["default"], rs["unsorted"]
    assert uns["diag"]["formulation"] == nle.MODE_PHI_FREE and uns["ev"].size == base["ev"].size
    Yu = uns["Y"].astype(np.float64)
    e_eig = rel_l2(base["ev"], uns["ev"])
    l2 = [rel_l2(base["Y"][j], Yu[j]) for j in range(L)]
    ex = excess(base["Y"], Yu, Yu, np.ones(Yu.shape[1:], dtype=bool))
    print("\nwide_rows %s sorted against unsorted: eigenvalues %.2e  layers rel L2 %s  per-pixel excess %s" % (case, e_eig, _fmt(l2), _fmt(ex)))
    _note_findings(case, "against the unsorted kernels", ex)
    assert e_eig < 1e-9, e_eig
    assert max(l2) < 1e-6, l2
    for j, e in enumerate(ex):
        assert e <= CAP, "layer %d: a pixel is %.3e max|Y| beyond one fp32 ulp of the unsorted kernels (bound %.1e)" % (j, e, CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SORTED)
def test_forced_forms_agree_with_the_default_run(nle, ctx, monkeypatch, case):
    """NLE_SORTED_TABLE turns the moment pass and the recurrence off, NLE_SORTED_NO_MOMENTS + NLE_GRAM_PAIRS the moment pass
    and the index-sum Gram: every case sits inside the predicates, so both change the arithmetic (other bits somewhere in
    eigenvalues or layers: the sorted kernels are bitwise reproducible) and neither may change the result"""
    rs = runs(nle, ctx, monkeypatch, case)
    base = rs["default"]
    for name in ("table", "forced"):
        r = rs[name]
        assert r["diag"]["formulation"] == nle.MODE_PHI_FREE and r["ev"].size == base["ev"].size
        e_eig = rel_l2(r["ev"], base["ev"])
        l2 = [rel_l2(r["Y"][j], base["Y"][j]) for j in range(L)]
        same = r["ev"].tobytes() == base["ev"].tobytes() and r["Y"].tobytes() == base["Y"].tobytes()
        print("wide_rows %s %s against default: bitwise %s  eigenvalues %.2e  layers rel L2 %s" % (case, name, same, e_eig, _fmt(l2)))
        assert not same, "%s: a reformulation should be on here, yet the plain forms give the same bits" % name
        assert e_eig < 1e-10, (name, e_eig)
        assert max(l2) < 1e-7, (name, l2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SORTED)
def test_the_default_run_is_bitwise_reproducible(nle, ctx, monkeypatch, case):
    rs = runs(nle, ctx, monkeypatch, case)
    assert rs["again"]["ev"].tobytes() == rs["default"]["ev"].tobytes()
    assert rs["again"]["Y"].tobytes() == rs["default"]["Y"].tobytes()


# --------------------------------------------------------------------------- GPU: expand around the layer switch
@pytest.mark.gpu
@pytest.mark.parametrize("case,n_layers", [(c, n) for c, ls in LAYER_CASES.items() for n in ls])
def test_expand_on_either_side_of_the_layer_switch(nle, ctx, monkeypatch, case, n_layers):
    """4096 columns and up to 12 sample columns: four layers per launch (L = 4 a full launch, 5 a full one and a rest);
    4097 columns, or 13 sample columns: two per launch.  Every layer against the oracle at the bars above."""
    s, r = setup(case), runs(nle, ctx, monkeypatch, case)["default"]
    Y, Y_o = r["layers"][n_layers], oracle_layers(case, n_layers)
    l2 = [rel_l2(Y[j], Y_o[j]) for j in range(n_layers)]
    ex = excess(Y, Y_o, Y_o, s["regions"]["plane"])
    print("\nwide_rows %s apply_layers(%d) against the oracle: rel L2 %s  per-pixel excess %s" % (case, n_layers, _fmt(l2), _fmt(ex)))
    _note_findings(case, "apply_layers(%d)" % n_layers, ex)
    assert np.isfinite(Y).all() and max(l2) < 1e-4, l2
    assert max(ex) <= CAP, ex
    if n_layers == L:
        assert Y.tobytes() == r["Y"].tobytes()


# ------------------------------------------------------------------------------ GPU: the plane back from its rows
@pytest.mark.gpu
@pytest.mark.parametrize("case", REBUILD_CASES)
def test_v_from_the_rebuilt_plane_is_v_from_the_kept_copy(nle, ctx, monkeypatch, case):
    """eigvecs() on a sorted-path filter projects V from the plane k_rows_from_sorted rebuilds (chunks of up to 32 pixels;
    whole rows from the sample values in the narrow cases); the unsorted filter projects it from its copy of the caller's
    plane.  At hy = 100 a level off by one moves a row of K by at least 1e-4 relative: a hundred times the bar."""
    rs = runs(nle, ctx, monkeypatch, case)
    V, V_ref = rs["default"]["V"].astype(np.float64), rs["unsorted"]["V"].astype(np.float64)
    assert V.shape == V_ref.shape == (H * setup(case)["W"], setup(case)["K"])
    sign = np.sign((V * V_ref).sum(0))
    assert (sign != 0).all()
    d, n = np.linalg.norm(V * sign - V_ref, axis=1), np.linalg.norm(V_ref, axis=1)
    assert n.min() > 0
    worst = int((d / n).argmax())
    print("\nwide_rows %s V from the rebuilt plane against V from the kept copy: worst row %d (image row %d, column %d) |dV| / |V| %.2e"
          % (case, worst, worst // setup(case)["W"], worst % setup(case)["W"], (d / n).max()))
    assert (d <= 1e-6 * n).all(), (worst, float((d / n).max()))


# -------------------------------------------------------------------------------- GPU: several planes in one walk
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PLANES_CASES))
def test_apply_planes_is_the_single_calls_bit_for_bit(nle, ctx, monkeypatch, case):
    pl = runs(nle, ctx, monkeypatch, case)["default"]["planes"]
    per_launch = 4 if setup(case)["nc"] <= 12 else 2
    assert pl["launches"] == 2 * -(-pl["P"] // per_launch), pl["launches"]     # both out kinds, on k_sorted_reduce_planes
    for kind in (0, 1):
        a, b = pl["batch"][kind], pl["single"][kind]
        assert a.shape == b.shape
        for m in range(pl["P"]):
            assert np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32)), (case, kind, m)


# ---------------------------------------------------------------------------------- GPU: training's reduce half
@pytest.mark.gpu
def test_apply_with_and_without_trainings_reduce_half(nle, ctx, monkeypatch):
    """apply(x_train) on the filter that kept training's reduce half against the filter trained and applied with
    set_train_reduce(False), and against the switch set at apply time alone: the same bits (test_apply_reuse.py)"""
    rs = runs(nle, ctx, monkeypatch, REUSE_CASE)
    on, off = rs["default"], rs["reuse_off"]
    assert np.array_equal(on["ev"], off["ev"])
    assert on["Y"].tobytes() == off["Y"].tobytes()
    assert on["apply"].tobytes() == off["apply"].tobytes()
    assert on["apply_off_at_apply"].tobytes() == on["apply"].tobytes()


# ---------------------------------------------------------------------------------------- GPU: the row pipeline
@pytest.mark.gpu
def test_second_rows_of_a_workgroup_with_another_slot_size(nle, oracle, ctx, monkeypatch):
    """W = 8192, nC = 10, nr = 4, H = CUs + 9 under NLE_SORTED_WGS_PER_CU=1: nine workgroups of every sorted kernel take a
    second row, and with rows cycling through seven kinds (CHP 32 / 16 / 24 / 20 ...) the descriptor read two rows ahead has
    another slot size than the row in hand.  No oracle at this size: sorted against unsorted, and a second sorted run."""
    W, nc, nr = 8192, 10, 4
    rows = n_cus() + 9
    sel_r, sel_c = oracle.sample_grid(rows, W, nr, nc)
    x, kinds = make_plane(TALL_ORDER, W, rows, sel_r, sel_c)
    samples = np.zeros((rows, W), dtype=bool)
    samples[np.ix_(sel_r, sel_c)] = True
    chp = [chunking(x[r], samples[r])["CHP"] for r in range(rows)]
    second = [(r - n_cus(), r) for r in range(n_cus(), rows)]
    assert len(second) == 9 and sum(chp[a] != chp[b] for a, b in second) >= 5 and max(chp) == 32, [(chp[a], chp[b]) for a, b in second]
    s = dict(x=x, nr=nr, nc=nc, hx=W / 8.0, K=8)
    x32 = x.astype(np.float32)

    def run(env, value="1"):
        _env(monkeypatch, env, value)
        try:
            f = nle.NLEFilter(ctx).train_filter(x32, nr, nc, s["hx"], HY, T, s["K"])
            try:
                assert f.diag()["formulation"] == nle.MODE_PHI_FREE
                return f.eigvals.copy(), _layers(f, x32, L, x32.shape)
            finally:
                f.close()
        finally:
            _env(monkeypatch, ())

    ev, Y = run(("NLE_SORTED_WGS_PER_CU",))
    ev2, Y2 = run(("NLE_SORTED_WGS_PER_CU",))
    ev_u, Y_u = run(UNSORTED)
    Yu = Y_u.astype(np.float64)
    e_eig = rel_l2(ev, ev_u)
    l2 = [rel_l2(Y[j], Yu[j]) for j in range(L)]
    ex = excess(Y, Yu, Yu, np.ones(Yu.shape[1:], dtype=bool))
    print("\nwide_rows tall %d x %d sorted (one workgroup per CU) against unsorted: eigenvalues %.2e  layers rel L2 %s  per-pixel excess %s"
          % (rows, W, e_eig, _fmt(l2), _fmt(ex)))
    _note_findings("tall", "against the unsorted kernels", ex)
    assert ev.size == ev_u.size == s["K"] and np.isfinite(Y).all()
    assert e_eig < 1e-9, e_eig
    assert max(l2) < 1e-6, l2
    assert max(ex) <= CAP, ex
    assert ev2.tobytes() == ev.tobytes() and Y2.tobytes() == Y.tobytes()


@pytest.fixture(scope="module", autouse=True)
def _drop_runs():
    yield
    _RUNS.clear()
