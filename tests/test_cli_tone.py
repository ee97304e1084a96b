"""The base tone curve's rows of the command-line option table (host/cli_common.hpp): --shadows, --highlights, --auto-levels,
--equalise (CPU only, no library).  The driver of tests/test_cli_options.py with the tone fields in its dump: a refusal is
exit status 2 and one line on stderr, an accepted line is the dump of the parsed fields."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "nonlocal-image-edit_amd")

DRIVER = r"""
#include <cstring>
#include <iostream>
#include "cli_common.hpp"

int main(int argc, char* argv[]) {
    const bool den = std::strcmp(argv[1], "denoise") == 0;   // argv[1]: the tool; the rest is its command line
    static char prog[] = "tool";
    argv[1] = prog;
    --argc, ++argv;
    nlecli::FilterArgs a;
    if (!nlecli::parse(argc, argv, den ? 12 : 10, &a, den ? nlecli::Tool::Denoise : nlecli::Tool::Enhance)) {
        std::cout << "usage" << std::endl;
        return 0;
    }
    std::cout.precision(17);
    std::cout << "tone=" << a.tone.shadows << "," << a.tone.highlights << "," << a.tone.clipPercent << "," << a.tone.equalise
              << " active=" << a.tone.active() << " line=" << a.toneLine << " detail=" << a.detail.residualWeight << "," << a.detail.gain
              << "," << a.detail.sigma << " radius=" << a.patchRadius << " sampler=" << a.sampler << " exact=" << a.exact
              << " chroma=" << a.chroma << " deep=" << a.deep << " report=" << a.nystromReport << " extra=" << a.extra.size()
              << std::endl;
    return 0;
}
"""

TAIL = "in.png out.png 3 4 5.5 6.5 7 8 1 2"
DTAIL = "in.png out.png 3 4 5.5 6.5 7 8 9 10 0.5"
REST = " detail=0,1,0 radius=0 sampler=0 exact=0 chroma=0 deep=0 report=0 extra=2\n"
ELSEWHERE = " is not supported here: the base tone curve remaps a layer, which this tool does not take\n"
COMBINE = " does not combine with --region or --tonemap: the base tone curve is built for the plain 8-bit and 16-bit enhance\n"
TAKES = {"--shadows": "--shadows takes a finite number in [-1, 1]", "--highlights": "--highlights takes a finite number in [-1, 1]",
         "--auto-levels": "--auto-levels takes a finite number in [0, 25]", "--equalise": "--equalise takes a finite number in [0, 1]"}


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """(tool, command line) -> (exit status, stderr, stdout) of the driver"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("cli_tone")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(PKG_DIR, "host"), str(d / "drv.cpp"), "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]   # cli_common.hpp alone: it links without the library

    def run(tool, line):
        r = subprocess.run([str(d / "drv"), tool] + line.split(), capture_output=True, text=True, timeout=30)
        return r.returncode, r.stderr, r.stdout
    return run


GOOD = [
    ("", "tone=0,0,-1,0 active=0 line=0"),
    ("--shadows 0.5", "tone=0.5,0,-1,0 active=1 line=0"),
    ("--shadows -1", "tone=-1,0,-1,0 active=1 line=0"),
    ("--shadows 1", "tone=1,0,-1,0 active=1 line=0"),
    ("--shadows 0", "tone=0,0,-1,0 active=0 line=0"),
    ("--highlights -0.25", "tone=0,-0.25,-1,0 active=1 line=0"),
    ("--highlights 1", "tone=0,1,-1,0 active=1 line=0"),
    ("--highlights -1", "tone=0,-1,-1,0 active=1 line=0"),
    ("--auto-levels 0", "tone=0,0,0,0 active=1 line=1"),
    ("--auto-levels 25", "tone=0,0,25,0 active=1 line=1"),
    ("--auto-levels 1.5", "tone=0,0,1.5,0 active=1 line=1"),
    ("--equalise 0", "tone=0,0,-1,0 active=0 line=1"),
    ("--equalise 1", "tone=0,0,-1,1 active=1 line=1"),
    ("--equalise 0.5", "tone=0,0,-1,0.5 active=1 line=1"),
    ("--equalise 0.5 --auto-levels 1 --highlights -0.5 --shadows 0.75", "tone=0.75,-0.5,1,0.5 active=1 line=1"),
    ("--shadows 0.25 --shadows 0.5", "tone=0.5,0,-1,0 active=1 line=0"),
]


def test_good_values_reach_the_fields(parse):
    for lead, dump in GOOD:
        assert parse("enhance", (lead + " " + TAIL).strip()) == (0, "", dump + REST), lead


def test_they_combine_with_the_other_enhance_options(parse):
    lead = ("--patch-radius 1 --sampler farthest --chroma 3 --deep --nystrom-report --residual-weight 1 --detail-gain 2 --detail-sigma 4 "
            "--shadows 0.5 --highlights -0.5 --auto-levels 2 --equalise 0.25")
    assert parse("enhance", lead + " " + TAIL) == (0, "", "tone=0.5,-0.5,2,0.25 active=1 line=1 detail=1,2,4 radius=1 sampler=1 exact=0 chroma=3 "
                                                          "deep=1 report=1 extra=2\n")
    assert parse("enhance", "--exact --equalise 1 " + TAIL) == (0, "", "tone=0,0,-1,1 active=1 line=1 detail=0,1,0 radius=0 sampler=0 exact=1 "
                                                                       "chroma=0 deep=0 report=0 extra=2\n")


BAD = [("--shadows", ["", "x", "nan", "inf", "1.01", "-1.5", "0.5x"]), ("--highlights", ["", "nan", "-inf", "1.0001", "-2"]),
       ("--auto-levels", ["", "-1", "-0.001", "25.5", "nan", "inf", "p"]), ("--equalise", ["", "-0.1", "1.1", "nan", "half"])]


def test_out_of_range_values_are_refused(parse):
    for name, values in BAD:
        for v in values:
            line = name + " " + TAIL if v == "" else "%s %s %s" % (name, v, TAIL)
            got = "in.png" if v == "" else v
            assert parse("enhance", line) == (2, "tool: %s, got '%s'\n" % (TAKES[name], got), ""), (name, v)
        assert parse("enhance", name) == (2, "tool: %s, got ''\n" % TAKES[name], ""), name


def test_denoise_refuses_them(parse):
    for name in TAKES:
        for line in (name + " 0.5 " + DTAIL, name + " x " + DTAIL, name):
            assert parse("denoise", line) == (2, "tool: " + name + ELSEWHERE, ""), line


def test_region_and_tonemap_are_refused_with_them(parse):
    for name in TAKES:
        assert parse("enhance", "%s 0.5 --region m.png:1,2 %s" % (name, TAIL)) == (2, "tool: " + name + COMBINE, ""), name
        assert parse("enhance", "--region m.png:1,2 %s 0.5 %s" % (name, TAIL)) == (2, "tool: " + name + COMBINE, ""), name
        assert parse("enhance", "--tonemap %s 0.5 in.hdr out.png 3 4 5.5 6.5 7 8 1 2" % name) == (2, "tool: " + name + COMBINE, ""), name
    # the last one given is named, and an inactive value is refused like an active one
    assert parse("enhance", "--shadows 0.5 --equalise 0.5 --region m.png:1,2 " + TAIL) == (2, "tool: --equalise" + COMBINE, "")
    assert parse("enhance", "--shadows 0 --tonemap in.hdr out.png 3 4 5.5 6.5 7 8 1 2") == (2, "tool: --shadows" + COMBINE, "")


def test_more_weights_than_layers_are_refused(parse):
    seventeen = " ".join(["1"] * 17)
    assert parse("enhance", "--highlights 0.5 in.png out.png 3 4 5.5 6.5 7 8 " + seventeen) == (
        2, "tool: --highlights takes at most 16 weights, got 17\n", "")
    sixteen = " ".join(["1"] * 16)
    assert parse("enhance", "--highlights 0.5 in.png out.png 3 4 5.5 6.5 7 8 " + sixteen)[0] == 0
    assert parse("enhance", "--highlights 0 in.png out.png 3 4 5.5 6.5 7 8 " + seventeen)[0] == 0      # inactive: the plain method's count
