"""`enhance --local-auto ROW:levels=P[,equalise=A]` (host/cli_common.hpp): the option table line by
line with a driver like tests/test_cli_local.py's over cli_common.hpp alone (CPU, no library), which dumps the parsed fields
and, row by row, the nle::LocalEdit that nlecli::local_edit_row resolves; then a few lines through the real tool on the GPU:
the `Tone curve: row` lines, the bytes of the C++ surface, and -- without the option -- the bytes the same commands wrote
before the option existed (tests/golden/local_auto_parent.json, recorded with the parent build on an MI355X).

A refusal is status 2 and the exact stderr text."""
import hashlib
import json
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")

DRIVER = r"""
#include <cstring>
#include <iostream>
#include <stdexcept>
#include "cli_common.hpp"

int main(int argc, char* argv[]) {
    const bool den = std::strcmp(argv[1], "denoise") == 0;   // argv[1]: the tool; the rest is its command line
    static char prog[] = "tool";
    argv[1] = prog;
    --argc, ++argv;
    nlecli::FilterArgs a;
    bool ok = false;
    try {
        ok = nlecli::parse(argc, argv, den ? 12 : 10, &a, den ? nlecli::Tool::Denoise : nlecli::Tool::Enhance);
    } catch (const std::invalid_argument&) {
        std::cout << "invalid_argument" << std::endl;
        return 3;
    }
    if (!ok) {
        std::cout << "usage" << std::endl;
        return 0;
    }
    std::cout.precision(17);
    std::cout << "locals=" << a.locals.size() << " autos=" << a.localAutos.size();
    for (const auto& u : a.localAutos)
        std::cout << " [" << u.text << " row=" << u.row << " has=" << u.hasLevels << u.hasEqualise << " levels=" << u.levels
                  << " equalise=" << u.equalise << " combine_row=" << nlecli::local_auto_row(a, u) << "]";
    std::cout << " rows:";
    for (int row = 0; row <= (int)a.locals.size(); ++row) {
        const nle::LocalEdit e = nlecli::local_edit_row(a, row);
        std::cout << " {t=" << e.shadows << "," << e.highlights << " P=" << e.clipPercent << " A=" << e.equalise << " s=" << e.saturation << "}";
    }
    std::cout << std::endl;
    return 0;
}
"""


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """(tool, command line) -> (exit status, stderr, stdout) of the driver"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("cli_local_auto")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(PKG_DIR, "host"), str(d / "drv.cpp"), "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]   # cli_common.hpp alone: it links without the library

    def run(tool, line):
        r = subprocess.run([str(d / "drv"), tool] + line.split(), capture_output=True, text=True, timeout=30)
        return r.returncode, r.stderr, r.stdout
    return run


TAIL = " in.png out.png 3 4 5.5 6.5 7 8 1 2"
TAILD = " in.png out.png 3 4 5.5 6.5 7 8 9 10 0.5"
PLAIN = "{t=0,0 P=-1 A=0 s=1}"
TAKES = "tool: --local-auto takes ROW:levels=P[,equalise=A] (a row number, then at least one of the two keys), got '%s'\n"
ROWTEXT = "a row is a whole number in [0, 8], 0 the background and m the m-th --local"
COMBINE = ("tool: --local does not combine with --region, --segment-weights, --tonemap, --auto-levels or --equalise: a region has one "
           "kind of edit, and a whole-image histogram has no per-region meaning yet\n")
L1 = "--local m.png:gain=1 "

# (tool, command line, exit status, stderr, stdout)
CASES = [
    # accepted: either key alone, both in both orders, the background's row, rows of masks and of segments, every field
    ("enhance", L1 + "--local-auto 1:levels=1" + TAIL, 0, "",
     "locals=1 autos=1 [1:levels=1 row=1 has=10 levels=1 equalise=0 combine_row=1] rows: " + PLAIN + " {t=0,0 P=1 A=0 s=1}\n"),
    ("enhance", L1 + "--local-auto 1:equalise=0.5" + TAIL, 0, "",
     "locals=1 autos=1 [1:equalise=0.5 row=1 has=01 levels=-1 equalise=0.5 combine_row=1] rows: " + PLAIN + " {t=0,0 P=-1 A=0.5 s=1}\n"),
    ("enhance", L1 + "--local-auto 0:levels=0,equalise=1" + TAIL, 0, "",
     "locals=1 autos=1 [0:levels=0,equalise=1 row=0 has=11 levels=0 equalise=1 combine_row=0] rows: {t=0,0 P=0 A=1 s=1} " + PLAIN + "\n"),
    ("enhance", "--local-auto 1:equalise=0,levels=25 " + L1 + TAIL, 0, "",
     "locals=1 autos=1 [1:equalise=0,levels=25 row=1 has=11 levels=25 equalise=0 combine_row=1] rows: " + PLAIN + " {t=0,0 P=25 A=0 s=1}\n"),
    ("enhance", "--shadows 0.5 --saturation 2 --local a.png:shadows=0 --local b.png:saturation=0 --local-auto 2:levels=2.5 --local-auto 0:equalise=0.25"
     + TAIL, 0, "",
     "locals=2 autos=2 [2:levels=2.5 row=2 has=10 levels=2.5 equalise=0 combine_row=2] [0:equalise=0.25 row=0 has=01 levels=-1 equalise=0.25 "
     "combine_row=0] rows: {t=0.5,0 P=-1 A=0.25 s=2} {t=0,0 P=-1 A=0 s=2} {t=0.5,0 P=2.5 A=0 s=0}\n"),
    # the issue's example: ROW counts the --local options, the combine's row of a segment target is its segment + 1
    ("enhance", "--segments 3 --local @0:shadows=0.5 --local @2:gain=0.5,sigma=6 --local-auto 1:levels=1,equalise=0.4 in.png out.png 20 20 30 30 10 50 3 3 1 1",
     0, "", "locals=2 autos=1 [1:levels=1,equalise=0.4 row=1 has=11 levels=1 equalise=0.40000000000000002 combine_row=1] rows: " + PLAIN +
     " {t=0.5,0 P=1 A=0.40000000000000002 s=1} " + PLAIN + "\n"),
    ("enhance", "--segments 4 --local @3:shadows=0.5 --local @1:highlights=0.5 --local-auto 2:levels=1 --local-auto 1:levels=3" + TAIL, 0, "",
     "locals=2 autos=2 [2:levels=1 row=2 has=10 levels=1 equalise=0 combine_row=2] [1:levels=3 row=1 has=10 levels=3 equalise=0 combine_row=4] "
     "rows: " + PLAIN + " {t=0.5,0 P=3 A=0 s=1} {t=0,0.5 P=1 A=0 s=1}\n"),
    ("enhance", "--deep --local-auto 1:levels=1 --region-spread 2 " + L1 + TAIL, 0, "",
     "locals=1 autos=1 [1:levels=1 row=1 has=10 levels=1 equalise=0 combine_row=1] rows: " + PLAIN + " {t=0,0 P=1 A=0 s=1}\n"),
    # the shape
    ("enhance", "--local-auto", 2, TAKES % "", ""),
    ("enhance", L1 + "--local-auto 1" + TAIL, 2, TAKES % "1", ""),
    ("enhance", L1 + "--local-auto 1:" + TAIL, 2, TAKES % "1:", ""),
    ("enhance", L1 + "--local-auto :levels=1" + TAIL, 2, TAKES % ":levels=1", ""),
    ("enhance", L1 + "--local-auto 1:levels" + TAIL, 2, TAKES % "1:levels", ""),
    ("enhance", L1 + "--local-auto 1:=1" + TAIL, 2, TAKES % "1:=1", ""),
    ("enhance", L1 + "--local-auto 1:levels=1," + TAIL, 2, TAKES % "1:levels=1,", ""),
    # ROW out of range: not a row number at all, and more than the --local options there are
    ("enhance", L1 + "--local-auto 9:levels=1" + TAIL, 2, "tool: --local-auto 9:levels=1: " + ROWTEXT + "\n", ""),
    ("enhance", L1 + "--local-auto -1:levels=1" + TAIL, 2, "tool: --local-auto -1:levels=1: " + ROWTEXT + "\n", ""),
    ("enhance", L1 + "--local-auto x:levels=1" + TAIL, 2, "tool: --local-auto x:levels=1: " + ROWTEXT + "\n", ""),
    ("enhance", L1 + "--local-auto m.png:levels=1" + TAIL, 2, "tool: --local-auto m.png:levels=1: " + ROWTEXT + "\n", ""),
    ("enhance", L1 + "--local-auto 2:levels=1" + TAIL, 2,
     "tool: --local-auto 2:levels=1: there are 2 rows, 0 the background and m the m-th --local\n", ""),
    ("enhance", "--local-auto 3:equalise=1 --segments 5 --local @4:gain=1 --local @0:gain=1" + TAIL, 2,
     "tool: --local-auto 3:equalise=1: there are 3 rows, 0 the background and m the m-th --local\n", ""),
    # a row given twice
    ("enhance", L1 + "--local-auto 1:levels=1 --local-auto 1:equalise=0.5" + TAIL, 2, "tool: --local-auto can be given once per row, row 1 has two\n", ""),
    ("enhance", L1 + "--local-auto 0:levels=1 --local-auto 1:levels=1 --local-auto 0:levels=1" + TAIL, 2,
     "tool: --local-auto can be given once per row, row 0 has two\n", ""),
    # keys and their values
    ("enhance", L1 + "--local-auto 1:shadows=0.5" + TAIL, 2, "tool: --local-auto 1:shadows=0.5: unknown key 'shadows' (the keys are levels, equalise)\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=1,Equalise=1" + TAIL, 2,
     "tool: --local-auto 1:levels=1,Equalise=1: unknown key 'Equalise' (the keys are levels, equalise)\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=1,levels=2" + TAIL, 2, "tool: --local-auto 1:levels=1,levels=2: key 'levels' is given twice\n", ""),
    ("enhance", L1 + "--local-auto 1:equalise=1,levels=2,equalise=1" + TAIL, 2,
     "tool: --local-auto 1:equalise=1,levels=2,equalise=1: key 'equalise' is given twice\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=25.5" + TAIL, 2, "tool: --local-auto 1:levels=25.5: levels takes a finite number in [0, 25], got '25.5'\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=-1" + TAIL, 2, "tool: --local-auto 1:levels=-1: levels takes a finite number in [0, 25], got '-1'\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=nan" + TAIL, 2, "tool: --local-auto 1:levels=nan: levels takes a finite number in [0, 25], got 'nan'\n", ""),
    ("enhance", L1 + "--local-auto 1:levels=" + TAIL, 2, "tool: --local-auto 1:levels=: levels takes a finite number in [0, 25], got ''\n", ""),
    ("enhance", L1 + "--local-auto 1:equalise=1.5" + TAIL, 2, "tool: --local-auto 1:equalise=1.5: equalise takes a finite number in [0, 1], got '1.5'\n", ""),
    ("enhance", L1 + "--local-auto 1:equalise=-0.1" + TAIL, 2, "tool: --local-auto 1:equalise=-0.1: equalise takes a finite number in [0, 1], got '-0.1'\n", ""),
    ("enhance", L1 + "--local-auto 1:equalise=x" + TAIL, 2, "tool: --local-auto 1:equalise=x: equalise takes a finite number in [0, 1], got 'x'\n", ""),
    # no --local, and the other tool
    ("enhance", "--local-auto 0:levels=1" + TAIL, 2,
     "tool: --local-auto needs at least one --local (ROW 0 is its background, ROW m the m-th --local)\n", ""),
    ("enhance", "--auto-levels 1 --local-auto 1:levels=1" + TAIL, 2,
     "tool: --local-auto needs at least one --local (ROW 0 is its background, ROW m the m-th --local)\n", ""),
    ("denoise", "--local-auto 1:levels=1" + TAILD, 2,
     "tool: --local-auto is not supported here: local adjustments edit layers and colour per region, which this tool does not take\n", ""),
    # the whole-image options stay refused beside --local, with or without the new option
    ("enhance", L1 + "--local-auto 1:levels=1 --auto-levels 1" + TAIL, 2, COMBINE, ""),
    ("enhance", "--equalise 0.5 " + L1 + "--local-auto 0:equalise=0.5" + TAIL, 2, COMBINE, ""),
    ("enhance", L1 + "--auto-levels 1" + TAIL, 2, COMBINE, ""),
    # without the option nothing is new
    ("enhance", L1 + TAIL, 0, "", "locals=1 autos=0 rows: " + PLAIN + " " + PLAIN + "\n"),
    ("enhance", "in.png out.png 3 4 5.5 6.5 7 8 1 2", 0, "", "locals=0 autos=0 rows: " + PLAIN + "\n"),
]


def test_every_line(parse):
    wrong = []
    for tool, line, status, err, out in CASES:
        got = parse(tool, line)
        if got != (status, err, out):
            wrong.append((tool, line, got, (status, err, out)))
    assert not wrong, "\n".join("%s %s\n  got  %r\n  want %r" % w for w in wrong[:10])


def test_the_list_is_whole():
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)   # no line twice
    text = " ".join(c[1] for c in CASES if c[2] == 0)
    assert "levels=" in text and "equalise=" in text and " @" in text and "m.png:" in text and "--local-auto 0:" in text
    assert sum(c[2] == 2 for c in CASES) >= 30


# ------------------------------------------------------------------------------------------------ GPU: the tool itself
SCENE_ARGV = ["6", "8", "30", "30", "10", "8"]
W4 = ["3.0", "3.0", "1.0", "0.9"]
CLI_BG = ["--residual-weight", "1", "--detail-gain", "2.5", "--detail-sigma", "6", "--shadows", "0.3", "--saturation", "1.25"]
CLI_SPECS = ["weights=2/2/1/1,gain=0.5,shadows=0.8,saturation=0", "residual=0,sigma=0,gain=1,highlights=-0.6", "shadows=0,saturation=2.5"]
MASK_AUTO = ["--local-auto", "1:levels=1,equalise=0.4", "--local-auto", "3:levels=0", "--local-auto", "0:equalise=0.3"]
SEG_LEAD = ["--segments", "3", "--local", "@0:shadows=0.5", "--local", "@2:gain=0.5,sigma=6"]
SEG_AUTO = ["--local-auto", "1:levels=1,equalise=0.4"]


def run_cli(lead, src, out):
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + SCENE_ARGV + W4, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


def pixels_sha256(path):
    from test_detail_curve import read_rgb8
    return hashlib.sha256(np.ascontiguousarray(read_rgb8(path)).tobytes()).hexdigest()


def mask_lead(masks):
    lead = list(CLI_BG)
    for m in range(3):
        lead += ["--local", masks[m] + ":" + CLI_SPECS[m]]
    return lead + ["--region-spread", "3", "--region-floor", "0.1"]


CPP = textwrap.dedent(r"""
    #include <cstdio>
    #include <iostream>
    #include <string>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #include "nle/image_io.hpp"
    #define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
    static void lines(const nle::NLEFilter& f, const std::vector<int>& rows, const std::vector<int>& combine) {
        const std::vector<nle::ToneLevels> t = f.lastLocalLevels();
        for (size_t k = 0; k < rows.size(); ++k)
            std::cout << "Tone curve: row " << rows[k] << " levels " << t.at(combine[k]).lo << " " << t.at(combine[k]).hi << std::endl;
    }
    int main(int argc, char** argv) {   // in out-masks out-segments mask0 mask1 mask2 out-segments-row0
        const nle::Image im = nle::imread(argv[1]);
        REQUIRE(!im.empty() && im.depth() == nle::NLE_8U && im.channels() == 3);
        std::vector<nle::Image> strokes;
        for (int m = 0; m < 3; ++m) {
            const nle::Image mask = nle::imread(argv[4 + m]);
            REQUIRE(!mask.empty());
            nle::Image s(mask.rows, mask.cols, nle::NLE_8U, 1);
            for (size_t i = 0; i < mask.total(); ++i) s.ptr<unsigned char>()[i] = mask.ptr<unsigned char>()[i * mask.channels()];
            strokes.push_back(s);
        }
        nle::NLEFilter f;
        f.verbose = false;
        f.keepTrainPlane = true;
        f.trainForEnhancement(im, 6, 8, 30, 30, 10, 8);
        nle::LocalEdit bg;                       // the rows of the mask command line in the test
        bg.weights = {3, 3, 1, 0.9};
        bg.detail.residualWeight = 1, bg.detail.gain = 2.5, bg.detail.sigma = 6;
        bg.shadows = 0.3, bg.saturation = 1.25;
        std::vector<nle::LocalEdit> edits(3, bg);
        edits[0].weights = {2, 2, 1, 1}, edits[0].detail.gain = 0.5, edits[0].shadows = 0.8, edits[0].saturation = 0;
        edits[1].detail = nle::DetailOptions(), edits[1].highlights = -0.6;
        edits[2].shadows = 0, edits[2].saturation = 2.5;
        REQUIRE(f.lastLocalLevels().empty());
        const nle::Image plain = f.enhanceLocal(im, strokes, edits, bg, 3, 0.1);
        REQUIRE(f.lastLocalLevels().empty());    // no row has levels or equalise: the calls it made before
        nle::LocalEdit bga = bg;
        bga.equalise = 0.3;
        edits[0].clipPercent = 1, edits[0].equalise = 0.4;
        edits[2].clipPercent = 0;
        const nle::Image out = f.enhanceLocal(im, strokes, edits, bga, 3, 0.1);
        REQUIRE(nle::imwrite(argv[2], out));
        const std::vector<nle::ToneLevels> t = f.lastLocalLevels();
        REQUIRE(t.size() == 4 && t[0].valid && t[1].valid && !t[2].valid && t[3].valid);
        std::cout << "masks" << std::endl;
        lines(f, {0, 1, 3}, {0, 1, 3});
        nle::LocalEdit bad = bg;
        bad.clipPercent = 26;
        try {
            f.enhanceLocal(im, strokes, {bad, bg, bg}, bg);
            REQUIRE(false);
        } catch (const std::runtime_error& e) {
            REQUIRE(std::string(e.what()).find("clipPercent") != std::string::npos);
        }
        // the segment command line: the background plain weights, segment 0 shadows 0.5 and the option, segment 2 a detail curve
        nle::SegmentOptions so;
        so.count = 3;
        f.segment(so);
        nle::LocalEdit sb;
        sb.weights = {3, 3, 1, 0.9};
        std::vector<nle::LocalEdit> se(3, sb);
        se[0].shadows = 0.5, se[0].clipPercent = 1, se[0].equalise = 0.4;
        se[2].detail.gain = 0.5, se[2].detail.sigma = 6;
        const nle::Image seg = f.enhanceSegmentsLocal(im, sb, se);
        REQUIRE(nle::imwrite(argv[3], seg));
        REQUIRE(f.lastLocalLevels().size() == 4 && f.lastLocalLevels()[1].valid && !f.lastLocalLevels()[0].valid);
        std::cout << "segments" << std::endl;
        lines(f, {1}, {1});
        // the same command with the option on ROW 0 alone: the background's row has it, no segment inherits it
        nle::LocalEdit sba = sb;
        sba.equalise = 0.3;
        std::vector<nle::LocalEdit> se0(3, sb);
        se0[0].shadows = 0.5;
        se0[2].detail.gain = 0.5, se0[2].detail.sigma = 6;
        const nle::Image seg0 = f.enhanceSegmentsLocal(im, sba, se0);
        REQUIRE(nle::imwrite(argv[7], seg0));
        const std::vector<nle::ToneLevels> t0 = f.lastLocalLevels();
        REQUIRE(t0.size() == 4 && t0[0].valid && !t0[1].valid && !t0[2].valid && !t0[3].valid);
        std::cout << "segments0" << std::endl;
        lines(f, {0}, {0});
        std::printf("auto OK\n");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    from PIL import Image
    from test_detail_curve import colour_scene
    from test_local_adjust import block_strokes, write_masks
    d = tmp_path_factory.mktemp("local_auto8")
    path = d / "in.bmp"
    Image.fromarray(np.ascontiguousarray(colour_scene()[..., ::-1])).save(path)
    return path, write_masks(d, block_strokes())


def tone_rows(stdout):
    return [l for l in stdout.splitlines() if l.startswith("Tone curve: row")]


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_tool_prints_the_rows_and_writes_the_bytes_of_the_cpp_surface(scene_files, tmp_path):
    from test_detail_curve import read_rgb8
    bmp, masks = scene_files
    host, libdir = os.path.join(PKG_DIR, "host"), os.path.join(PKG_DIR, "lib")
    (tmp_path / "drv.cpp").write_text(CPP)
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "NLE_DEVICES"}
    r = subprocess.run([str(tmp_path / "drv"), str(bmp), str(tmp_path / "drv.png"), str(tmp_path / "drvseg.png")] + masks + [str(tmp_path / "drvseg0.png")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "auto OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    drv = r.stdout.splitlines()
    drv_masks, drv_seg = drv[drv.index("masks") + 1:drv.index("segments")], drv[drv.index("segments") + 1:drv.index("segments0")]
    drv_seg0 = tone_rows("\n".join(drv[drv.index("segments0"):]))
    # masks: three rows have the option, given out of order; the lines come in ascending ROW
    out = run_cli(mask_lead(masks) + MASK_AUTO, bmp, tmp_path / "cli.png")
    rows = tone_rows(out)
    assert [l.split()[3] for l in rows] == ["0", "1", "3"] and rows == drv_masks, (rows, drv_masks)
    for l in rows:
        lo, hi = float(l.split()[5]), float(l.split()[6])
        assert -256 <= lo < hi <= 768
    assert float(rows[2].split()[5]) != 0.0                   # levels=0 on row 3: lo is the row's own
    assert np.array_equal(read_rgb8(tmp_path / "cli.png"), read_rgb8(tmp_path / "drv.png"))
    run_cli(mask_lead(masks), bmp, tmp_path / "plain.png")
    assert not np.array_equal(read_rgb8(tmp_path / "cli.png"), read_rgb8(tmp_path / "plain.png"))
    # segments: the issue's example
    out = run_cli(SEG_LEAD + SEG_AUTO, bmp, tmp_path / "cliseg.png")
    rows = tone_rows(out)
    assert len(rows) == 1 and rows == drv_seg and rows[0].startswith("Tone curve: row 1 levels ")
    assert np.array_equal(read_rgb8(tmp_path / "cliseg.png"), read_rgb8(tmp_path / "drvseg.png"))
    # ROW 0 in segment mode is the background's row alone: one line, and segment 1, which has no --local, does not inherit it
    out = run_cli(SEG_LEAD + ["--local-auto", "0:equalise=0.3"], bmp, tmp_path / "cliseg0.png")
    rows = tone_rows(out)
    assert len(rows) == 1 and rows == drv_seg0 and rows[0].startswith("Tone curve: row 0 levels ")
    assert np.array_equal(read_rgb8(tmp_path / "cliseg0.png"), read_rgb8(tmp_path / "drvseg0.png"))


@pytest.mark.gpu
def test_the_mask_command_equals_the_python_composition(nle, ctx, scene_files, tmp_path):
    from test_detail_curve import NL, ROUNDED8, colour_scene, read_rgb8, train_scene
    from test_local_adjust import PY_DETAIL, PY_SAT, PY_TONE, PY_W, block_strokes, stroke_scale
    bmp, masks = scene_files
    run_cli(mask_lead(masks) + MASK_AUTO, bmp, tmp_path / "cli.png")
    bgr = colour_scene()
    H, W = bgr.shape[:2]
    s = block_strokes()
    lab, L = ctx.bgr2lab8(bgr)
    f = train_scene(nle, ctx, L)
    auto = [(-1.0, 0.3), (1.0, 0.4), (-1.0, 0.0), (0.0, 0.0)]
    tone = [(PY_TONE[m][0], PY_TONE[m][1], auto[m][0], auto[m][1]) for m in range(4)]
    y, q = f.apply_local_auto(L, NL, s, PY_W, tone, PY_DETAIL, stroke_scale(s), 3.0, 0.1, ROUNDED8, want_spreads=True)
    a, b = ctx.lab8_channel(lab, 1).reshape(-1), ctx.lab8_channel(lab, 2).reshape(-1)
    ctx.local_chroma(a, b, q, PY_SAT, 0.1, out="inplace")
    want = ctx.lab2bgr8(lab, L=y.view(H, W), a=a.view(H, W), b=b.view(H, W)).cpu().numpy()
    f.close()
    assert np.array_equal(read_rgb8(tmp_path / "cli.png")[..., ::-1], want)


@pytest.mark.gpu
def test_without_the_option_the_commands_write_the_bytes_they_wrote_before(scene_files, tmp_path):
    """the same two command lines without --local-auto: the decoded pixels are those the build before this option wrote, and
    no `Tone curve` line appears"""
    bmp, masks = scene_files
    golden = json.load(open(os.path.join(GOLDEN, "local_auto_parent.json")))
    out = run_cli(mask_lead(masks), bmp, tmp_path / "masks.png")
    assert "Tone curve" not in out and pixels_sha256(tmp_path / "masks.png") == golden["masks"]
    out = run_cli(SEG_LEAD, bmp, tmp_path / "seg.png")
    assert "Tone curve" not in out and pixels_sha256(tmp_path / "seg.png") == golden["segments"]
