"""`enhance --segments C [--segment-spread T] [--segment-iterations I] [--segment-map FILE] [--segment-weights c:w1,w2,...]`
and the C++ surface behind it (NLEFilter::segment / enhanceSegments), against the Python mirror's composition

    bgr2lab8 -> train -> segment -> apply_layers -> region_combine (ROUNDED8) -> lab2bgr8

The rule itself is restated and tested in tests/test_segments.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_patch_affinity as tpa  # noqa: E402
import test_segments as tsg  # noqa: E402

ENHANCE, DENOISE = tpa.ENHANCE, tpa.DENOISE
FLOWER, FLOWER_ARGS, DENOISE_ARGS = tpa.FLOWER, tpa.FLOWER_ARGS, tpa.DENOISE_ARGS
FLOWER_BMP = os.path.join(GOLDEN, "flower-50.bmp")
FLOOR, ROUNDED8 = 0.05, 1
W0, W2 = [4.0, 3.0, 2.0, 1.0], [0.5, 0.5, 1.0, 1.0]
NINE = [v for c in range(9) for v in ("--segment-weights", f"{c % 8}:1,2,3,4")]

# (leading options, what the one line on stderr must hold)
REFUSALS = [
    (["--segments"], "--segments takes an integer in [2, 8]"),  # the next word is the image: no number
    (["--segments", "1"], "--segments takes an integer in [2, 8]"),
    (["--segments", "9"], "--segments takes an integer in [2, 8]"),
    (["--segments", "3.5"], "--segments takes an integer in [2, 8]"),
    (["--segments", "x"], "--segments takes an integer in [2, 8]"),
    (["--segments", "3", "--segment-spread", "0"], "--segment-spread takes a finite number > 0"),
    (["--segments", "3", "--segment-spread", "-1"], "--segment-spread takes a finite number > 0"),
    (["--segments", "3", "--segment-spread", "nan"], "--segment-spread takes a finite number > 0"),
    (["--segment-spread", "inf", "--segments", "3"], "--segment-spread takes a finite number > 0"),
    (["--segments", "3", "--segment-iterations", "0"], "--segment-iterations takes an integer in [1, 200]"),
    (["--segments", "3", "--segment-iterations", "201"], "--segment-iterations takes an integer in [1, 200]"),
    (["--segments", "3", "--segment-iterations", "1.5"], "--segment-iterations takes an integer in [1, 200]"),
    (["--segments", "3", "--segment-map", "--exact"], "--segment-map takes a file name"),
    (["--segments", "3", "--segment-weights", "0"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", "0:"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", ":1,2,3,4"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", "x:1,2,3,4"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", "-1:1,2,3,4"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "8", "--segment-weights", "8:1,2,3,4"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", "0:1,,3,4"], "--segment-weights takes c:w1,w2,..."),
    (["--segments", "3", "--segment-weights", "0:1,2,3,nan"], "--segment-weights takes c:w1,w2,..."),
    # the dependent options need --segments
    (["--segment-spread", "4"], "--segment-spread needs --segments"),
    (["--segment-iterations", "40"], "--segment-iterations needs --segments"),
    (["--segment-map", "m.png"], "--segment-map needs --segments"),
    (["--segment-weights", "0:1,2,3,4"], "--segment-weights needs --segments"),
    # a segment that does not exist, a segment twice, a weight count that is not the command line's
    (["--segments", "3", "--segment-weights", "3:1,2,3,4"], "there are 3 segments"),
    (["--segment-weights", "2:1,2,3,4", "--segments", "2"], "there are 2 segments"),
    (["--segments", "3", "--segment-weights", "1:1,2,3,4", "--segment-weights", "1:4,3,2,1"], "once per segment"),
    (["--segments", "8"] + NINE, "once per segment"),
    (["--segments", "3", "--segment-weights", "0:1,2,3"], "--segment-weights 0 has 3 weights, the command line has 4"),
    (["--segments", "3", "--segment-weights", "0:1,2,3,4,5"], "--segment-weights 0 has 5 weights, the command line has 4"),
    # what --region refuses, for the same reasons
    (["--segments", "3", "--region", "m.png:1,2,3,4"], "--segments does not combine with --region"),
    (["--region", "m.png:1,2,3,4", "--segments", "3"], "--segments does not combine with --region"),
    (["--segments", "3", "--deep"], "--segments does not combine with --region, --deep or --tonemap"),
    (["--tonemap", "--segments", "3"], "--segments does not combine with --region, --deep or --tonemap"),
    (["--segments", "3", "--residual-weight", "1"], "--residual-weight does not combine with --segments"),
    (["--segments", "3", "--detail-sigma", "2"], "--detail-sigma does not combine with --segments"),
    (["--detail-sigma", "2", "--detail-gain", "2", "--segments", "3"], "--detail-gain does not combine with --segments"),
    (["--segments", "3", "--shadows", "0.5"], "--shadows does not combine with --segments"),
    (["--segments", "3", "--highlights", "0.5"], "--highlights does not combine with --segments"),
    (["--auto-levels", "1", "--segments", "3"], "--auto-levels does not combine with --segments"),
    (["--segments", "3", "--equalise", "0.5"], "--equalise does not combine with --segments"),
]


@pytest.mark.parametrize("lead,text", REFUSALS, ids=lambda v: "_".join(v[:5]).replace("--", "") if isinstance(v, list) else None)
def test_cli_refuses_bad_segment_options_before_any_gpu_call(lead, text, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([ENHANCE] + lead + [FLOWER_BMP, str(out)] + FLOWER_ARGS, capture_output=True, text=True, timeout=60,
                       env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert text in r.stderr and r.stderr.count("\n") == 1, r.stderr
    assert r.stdout == "" and not out.exists() and not (tmp_path / "m.png").exists()


@pytest.mark.parametrize("lead", [["--segments", "3"], ["--segment-spread", "4"], ["--segment-iterations", "40"],
                                  ["--segment-map", "m.png"], ["--segment-weights", "0:2"]],
                         ids=lambda v: v[0].replace("--", ""))
def test_denoise_cli_refuses_segment_options_before_any_gpu_call(lead, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([DENOISE] + lead + [FLOWER_BMP, str(out)] + DENOISE_ARGS, capture_output=True, text=True, timeout=60,
                       env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert lead[0] + " is not supported here" in r.stderr
    assert r.stdout == "" and not out.exists()


def test_surface_declares_the_segment_methods():
    hpp = " ".join(open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nle", "filter.hpp")).read().split())
    for decl in ("struct SegmentOptions {", "int count = 0;", "double spread = 4;", "int maxIterations = 40;", "double floor = 0.05;",
                 "Image segment(const SegmentOptions& options);", "SegmentReport lastSegments() const",
                 "Image enhanceSegments(const Image& I, const std::vector<DType>& weights, "
                 "const std::vector<std::vector<DType>>& segmentWeights) const;"):
        assert decl in hpp, decl


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def sctx(ctx):
    """the session ctx, handed back in auto mode whatever the test did"""
    yield ctx
    ctx.set_mode(0)


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)).convert("RGB"))[..., ::-1]


def _segment_lines(stdout, Cn):
    """(iterations, converged, counts) of the lines `enhance --segments` adds"""
    head = re.search(r"^Segments: (\d+) iterations (\d+) converged (yes|no) objective (\S+)$", stdout, flags=re.M)
    assert head and int(head.group(1)) == Cn, stdout
    rows = re.findall(r"^Segment (\d+): (\d+) pixels, mean L (\S+)$", stdout, flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(Cn)), stdout
    return int(head.group(2)), head.group(3) == "yes", [int(r[1]) for r in rows], [float(r[2]) for r in rows], float(head.group(4))


def _mirror(nle, ctx, src, params, Cn, rows, exact=False):
    """the composition through the Python mirror: (BGR image, segment result, L plane)"""
    H, W = src.shape[:2]
    lab, L = ctx.bgr2lab8(src)
    if exact:
        ctx.set_mode(nle.MODE_EXACT_F64)
    f = nle.NLEFilter(ctx).train_filter(L, *params)
    r = f.segment(Cn, want_spreads=True)
    y = None
    if rows is not None:
        layers = f.apply_layers(L, len(rows[0]))
        y = ctx.region_combine(layers, r["spreads"], np.array(rows), FLOOR, ROUNDED8)
        y = ctx.lab2bgr8(lab, L=y.view(H, W)).cpu().numpy()
    f.close()
    return y, r, L


@pytest.mark.gpu
def test_enhance_segments_without_weights_writes_the_plain_image_and_the_map(nle, sctx, tmp_path):
    src = tpa._load_bgr("flower-50.bmp")
    H, W = src.shape[:2]
    plain, out, seg = tmp_path / "plain.png", tmp_path / "out.png", tmp_path / "m.png"
    r0 = subprocess.run([ENHANCE, FLOWER_BMP, str(plain)] + FLOWER_ARGS, capture_output=True, text=True, timeout=600)
    r = subprocess.run([ENHANCE, "--segments", "3", "--segment-map", str(seg), FLOWER_BMP, str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and r.returncode == 0, (r0.stderr, r.stderr)
    assert open(plain, "rb").read() == open(out, "rb").read()  # the combine is skipped: byte for byte the plain command
    assert r.stdout.startswith(r0.stdout)  # the lines are added behind what was there
    _, res, L = _mirror(nle, sctx, src, (FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"]), 3, None)
    labels = res["labels"].cpu().numpy()
    grey = _read(seg)
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])
    assert np.array_equal(grey[..., 0].ravel(), np.rint(255.0 * labels / 2).astype(np.uint8))
    iters, conv, counts, mean_l, J = _segment_lines(r.stdout, 3)
    assert counts == res["counts"].tolist() and iters == res["iterations"] and conv == res["converged"]
    assert abs(J - res["objective"][-1]) <= 1e-5 * abs(J)  # six digits are printed
    Lh = L.cpu().numpy().ravel().astype(np.float64)
    for c in range(3):
        assert abs(mean_l[c] - Lh[labels == c].mean()) <= 1e-5 * 255
    assert min(counts) > 0 and sum(counts) == H * W  # three segments that are there (position counts: two may be as light)


@pytest.mark.gpu
def test_enhance_with_segment_weights_matches_the_python_mirror(nle, sctx, tmp_path):
    src = tpa._load_bgr("flower-50.bmp")
    out = tmp_path / "out.png"
    r = subprocess.run([ENHANCE, "--segments", "3", "--segment-weights", "0:4,3,2,1", "--segment-weights", "2:0.5,0.5,1,1",
                        FLOWER_BMP, str(out)] + FLOWER_ARGS, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [FLOWER["weights"], W0, FLOWER["weights"], W2]  # the background, then segment 0, 1 (the positional weights) and 2
    mirror, res, _ = _mirror(nle, sctx, src, (FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"]), 3, rows)
    assert np.array_equal(_read(out), mirror)
    assert _segment_lines(r.stdout, 3)[2] == res["counts"].tolist()
    # and it is an edit of its own: not what the positional weights give everywhere
    plain, _, _ = _mirror(nle, sctx, src, (FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"]), 3,
                          [FLOWER["weights"]] * 4)
    assert not np.array_equal(mirror, plain)


@pytest.mark.gpu
def test_enhance_exact_with_segment_weights_matches_the_python_mirror(nle, sctx, tmp_path):
    """--exact on the three-block scene of tests/test_segments.py as a grey image (48 x 64: the exact train stays short)"""
    from PIL import Image
    x, truth = tsg._blocks()
    H, W, nr, nc, hx, hy, T, K = tsg.BLOCKS
    g = x.astype(np.uint8)
    src = np.stack([g, g, g], axis=-1)
    inp, out, seg = tmp_path / "blocks.png", tmp_path / "out.png", tmp_path / "m.png"
    Image.fromarray(src).save(str(inp))
    args = [str(nr), str(nc), str(hx), str(hy), str(T), str(K), "2", "3", "4", "1"]
    r = subprocess.run([ENHANCE, "--segment-weights", "1:4,3,2,1", "--exact", "--segment-map", str(seg), "--segments", "3",
                        str(inp), str(out)] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [[2.0, 3.0, 4.0, 1.0], [2.0, 3.0, 4.0, 1.0], W0, [2.0, 3.0, 4.0, 1.0]]
    mirror, res, _ = _mirror(nle, sctx, src, (nr, nc, hx, hy, T, K), 3, rows, exact=True)
    assert np.array_equal(_read(out), mirror)
    assert np.array_equal(_read(seg)[..., 0].ravel(), np.rint(255.0 * res["labels"].cpu().numpy() / 2).astype(np.uint8))
    assert _segment_lines(r.stdout, 3)[2] == res["counts"].tolist()
