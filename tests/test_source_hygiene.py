"""Housekeeping: the product kernels carry no measurement-only code paths (the ablation / timestamp variants of
k_sorted_pass behind profiles/r2_pass_ablation.txt lived beside the sources as a patch until round 4; the kernel they
patched has changed since -- its pixel loop runs on moments now -- and the patch went with it: the profile is the record)."""
import glob
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from conftest import PKG_DIR, ROOT


def test_product_sources_have_no_ablation_hooks():
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")) + glob.glob(os.path.join(PKG_DIR, "host", "*")):
        text = open(f, errors="replace").read()
        assert "NLE_ABL_" not in text and "NLE_STAMP" not in text, f


# Environment switches whose variants were taken out (nothing but the switch reached them): no source may read them again
REMOVED_SWITCHES = ("NLE_HIST_UNTILED", "NLE_PROJECT_HIST", "NLE_EAGER_V", "NLE_APPLY_WITH_V", "NLE_HOST_ORTHO",
                    "NLE_PROJECT_CHUNKED", "NLE_NO_SORTED_EXPAND",
                    # the solver layer's tuning and measurement switches
                    "NLE_DEVICE_TRIDIAG", "NLE_WA_SERIAL", "NLE_NO_DEFLATE", "NLE_HOST_THREADS", "NLE_EIG_TQL",
                    "NLE_EIG_NO_BLOCK", "NLE_EIG_NO_INVIT", "NLE_EIG_THREADS", "NLE_PIN_THREADS", "NLE_EIG_TRACE",
                    "NLE_SYTRD_CW", "NLE_SYTRD_PROBE",
                    # the multi-rank fault injection: no source reads it (the tests inject through the all-reduce callback)
                    "NLE_FAULT_RANK")


def test_product_sources_read_no_removed_switches():
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")) + glob.glob(os.path.join(PKG_DIR, "host", "*")):
        text = open(f, errors="replace").read()
        for name in REMOVED_SWITCHES:
            assert name not in text, (f, name)


# The per-site launch macros that csrc/launch.h's dispatch_values / dispatch_columns / launch() replaced: no source defines
# one again (a kernel that is instantiated per size is selected and launched through launch.h)
REMOVED_LAUNCH_MACROS = ("NLE_TS_CASE", "NLE_DISPATCH_Q", "NLE_DISPATCH_GQ", "NLE_T3", "NLE_SP_CASE", "NLE_G64", "NLE_PR",
                         "NLE_PJ_CASE", "NLE_RP64", "NLE_PATCH_LAUNCH", "NLE_RS_CASE", "NLE_SYW")


def test_product_sources_define_no_removed_launch_macros():
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")) + glob.glob(os.path.join(PKG_DIR, "host", "*")):
        text = open(f, errors="replace").read()
        for name in REMOVED_LAUNCH_MACROS:
            assert not re.search(r"\b%s\b" % name, text), (f, name)


def test_attribute_calls_live_in_launch_h_and_the_documented_exceptions():
    """the dynamic-LDS limit is raised by launch(); outside it only the once-per-process attribute of the residual map
    (resid.hip) and the one ahead of the chunk loop of the pair tables (tables.hip), and no macro launches a kernel"""
    calls = {}
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")):
        text = open(f, errors="replace").read()
        n = len(re.findall(r"hipFuncSetAttribute\s*\(", text))
        if n:
            calls[os.path.basename(f)] = n
        for body in re.findall(r"^[ \t]*#[ \t]*define[^\n]*(?:\\\n[^\n]*)*", text, flags=re.M):
            assert "hipLaunchKernelGGL" not in body and "hipFuncSetAttribute" not in body and "launch(" not in body, (f, body[:80])
    assert calls == {"launch.h": 1, "resid.hip": 1, "tables.hip": 1}, calls


DISPATCH_DRIVER = textwrap.dedent(r"""
    #include "launch.h"
    #include <cstdio>
    using namespace nlek;
    int main() {
        for (int v = -2; v <= 260; ++v) {   // a list with gaps: the multiples of 16 up to 256
            int calls = 0, got = -1;
            const bool r = dispatch_values<16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256>(
                v, [&](auto c) { ++calls, got = decltype(c)::value; });
            std::printf("L %d %d %d %d\n", v, (int)r, calls, got);
        }
        for (int v = 0; v <= 12; ++v) {     // a range
            int calls = 0, got = -1;
            const bool r = dispatch_columns<3, 9>(v, [&](auto c) { ++calls, got = decltype(c)::value; });
            std::printf("R %d %d %d %d\n", v, (int)r, calls, got);
        }
        for (int g = 0; g <= 66; ++g)       // two levels: a list inside a list
            for (int q = 0; q <= 9; ++q) {
                int calls = 0, gg = -1, gq = -1;
                bool inner = false;
                const bool r = dispatch_values<4, 8, 16, 32, 64>(g, [&](auto cg) {
                    inner = dispatch_values<1, 2, 4, 6, 7, 8>(q, [&](auto cq) { ++calls, gg = decltype(cg)::value, gq = decltype(cq)::value; });
                });
                std::printf("N %d %d %d %d %d %d\n", g, q, (int)(r && inner), calls, gg, gq);
            }
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dispatch_calls_once_for_a_listed_value_and_never_outside(tmp_path):
    """csrc/launch.h alone on the host: the list form and the range form call f exactly once, with the matching constant,
    for every listed value (lowest, highest, around each gap) and not at all outside, and say so in what they return"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    (tmp_path / "drv.cpp").write_text(DISPATCH_DRIVER)
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                        "-I", os.path.join(PKG_DIR, "csrc"), str(tmp_path / "drv.cpp"), "-o", str(tmp_path / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(tmp_path / "drv")], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in r.stdout.splitlines()]
    nkey = {"L": 1, "R": 1, "N": 2}   # a row: the form, the value(s) asked for, then what came back
    got = {(t[0], *map(int, t[1:1 + nkey[t[0]]])): tuple(map(int, t[1 + nkey[t[0]]:])) for t in rows}
    want = {}
    for v in range(-2, 261):
        want[("L", v)] = (1, 1, v) if v in range(16, 257, 16) else (0, 0, -1)
    for v in range(0, 13):
        want[("R", v)] = (1, 1, v) if 3 <= v <= 9 else (0, 0, -1)
    for g in range(0, 67):
        for q in range(0, 10):
            want[("N", g, q)] = (1, 1, g, q) if g in (4, 8, 16, 32, 64) and q in (1, 2, 4, 6, 7, 8) else (0, 0, -1, -1)
    assert len(rows) == len(want) and got == want, [(k, got.get(k), w) for k, w in want.items() if got.get(k) != w][:10]


# ---------------------------------------------------------------------------- the host algebra's files (csrc/*.cpp)
def test_every_host_source_is_built_into_the_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nle_build_recipe", os.path.join(PKG_DIR, "build.py"))
    recipe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recipe)
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*.cpp"))}
    assert on_disk and on_disk <= set(recipe.LIB_SOURCES), sorted(on_disk - set(recipe.LIB_SOURCES))


def test_tools_and_tests_link_the_host_sources_and_never_include_them():
    files = [f for d in ("tools", "tests") for f in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True) if os.path.isfile(f)]
    assert len(files) > 20
    names = "|".join(re.escape(os.path.basename(f)) for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*.cpp")))
    included = re.compile(r'#\s*include\s*[<"](?:[^>"\n]*/)?(?:%s)[>"]' % names)   # by any path, also through -I
    for f in files:
        assert not included.search(open(f, errors="replace").read()), f


def test_sym_eigen_select_is_internal():
    assert "sym_eigen_select" not in open(os.path.join(PKG_DIR, "csrc", "eigen_sym.h")).read()


# ---------------------------------------------------------------------------- the switches that remain: csrc/switches.h
SWITCHES_H = os.path.join(PKG_DIR, "csrc", "switches.h")
CLI_VARIABLES = ("NLE_MODE", "NLE_DEVICES", "NLE_DEVICE", "NLE_REPORT")


def test_the_environment_is_read_in_one_place():
    """under csrc/ only switches.h asks the environment; in host/ (the CLI layer, outside the library) every variable has
    exactly one reader"""
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")):
        if os.path.basename(f) != "switches.h":
            assert "getenv" not in open(f, errors="replace").read(), f
    host = "".join(open(f, errors="replace").read() for f in sorted(glob.glob(os.path.join(PKG_DIR, "host", "*"))))
    reads = re.findall(r'getenv\(\s*"([^"]*)"\s*\)', host)
    assert len(reads) == host.count("getenv"), "a getenv call in host/ whose argument is not a literal name"
    assert sorted(reads) == sorted(CLI_VARIABLES), reads


def switch_names():
    return set(re.findall(r'"(NLE_[A-Z0-9_]+)"', open(SWITCHES_H).read()))


def test_the_documented_switches_are_the_ones_read():
    """the table of INTEGRATION.md section 3 names exactly the variables switches.h reads, and none that was removed"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = re.findall(r"^\| `(NLE_[A-Z0-9_]+)` \|", text, flags=re.M)
    assert len(rows) == len(set(rows)), rows
    names = switch_names()
    assert len(names) == 20, sorted(names)
    assert set(rows) == names, (sorted(set(rows) - names), sorted(names - set(rows)))
    assert not names & set(REMOVED_SWITCHES) and not set(rows) & set(REMOVED_SWITCHES)
    for name in REMOVED_SWITCHES:
        assert name not in text, name


SWITCH_DRIVER = textwrap.dedent(r"""
    #include "switches.h"
    #include <cstdio>
    int main() {
        const nlesw::Switches s = nlesw::read_switches();
        std::printf("NLE_TRACE=%d\nNLE_FORCE_EIG=%d\nNLE_HOST_SOLVER=%d\nNLE_HOST_KA=%d\nNLE_HOST_WA=%d\nNLE_HOST_Q=%d\n",
                    s.trace, s.force_eig, s.host_solver, s.host_ka, s.host_wa, s.host_q);
        std::printf("NLE_DEV_SOLVER_MIN=%d\nsytrd_g_set=%d\nNLE_SYTRD_G=%d\nNLE_NYSTROM_BF16X3=%d\n", s.dev_solver_min,
                    s.sytrd_g_set, s.sytrd_g, s.nystrom_bf16x3);
        std::printf("NLE_NO_SORTED_ROWS=%d\nNLE_ALL_LEVEL_TILES=%d\nNLE_SORTED_TABLE=%d\nNLE_SORTED_NO_MOMENTS=%d\n"
                    "NLE_GRAM_PAIRS=%d\nNLE_SORTED_WGS_PER_CU=%d\n", s.no_sorted_rows, s.all_level_tiles, s.sorted_table,
                    s.sorted_no_moments, s.gram_pairs, s.sorted_wgs_per_cu);
        std::printf("NLE_AUTO_STREAM64=%d\nNLE_STREAM64_CHUNK_MB=%d\nNLE_Q_SOLVER=%d\nNLE_EIG_NO_BISECT=%d\nNLE_EIG_NO_X8=%d\n",
                    s.auto_stream64, s.stream64_chunk_mb, s.q_solver, s.eig_no_bisect, s.eig_no_x8);
        return 0;
    }
""")
FLAGS = ("NLE_TRACE", "NLE_FORCE_EIG", "NLE_HOST_SOLVER", "NLE_HOST_KA", "NLE_HOST_WA", "NLE_HOST_Q", "NLE_NYSTROM_BF16X3",
         "NLE_NO_SORTED_ROWS", "NLE_ALL_LEVEL_TILES", "NLE_SORTED_TABLE", "NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS",
         "NLE_AUTO_STREAM64", "NLE_EIG_NO_BISECT", "NLE_EIG_NO_X8")
DEFAULTS = dict({k: 0 for k in FLAGS}, NLE_DEV_SOLVER_MIN=288, sytrd_g_set=0, NLE_SYTRD_G=0, NLE_SORTED_WGS_PER_CU=2,
                NLE_STREAM64_CHUNK_MB=2048, NLE_Q_SOLVER=0)


@pytest.fixture(scope="module")
def read_switches(tmp_path_factory):
    """env -> the struct read_switches() fills in a child process that has exactly these NLE_* variables"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("switches")
    (d / "drv.cpp").write_text(SWITCH_DRIVER)
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG_DIR, "csrc"), str(d / "drv.cpp"),
                        "-o", str(d / "drv")], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-2000:]   # switches.h alone, no HIP, no other header of the library
    base = {k: v for k, v in os.environ.items() if not k.startswith("NLE_")}

    def run(**env):
        r = subprocess.run([str(d / "drv")], capture_output=True, text=True, timeout=30, env=dict(base, **env))
        assert r.returncode == 0, r.stderr
        return {k: int(v) for k, v in (line.split("=") for line in r.stdout.split())}
    return run


def test_switch_defaults(read_switches):
    got = read_switches()
    assert got == DEFAULTS
    assert set(got) - {"sytrd_g_set"} == switch_names()          # the driver prints every name the header reads


@pytest.mark.parametrize("value", ["1", "0", ""], ids=["one", "zero", "empty"])
def test_every_flag_is_on_when_its_name_is_present(read_switches, value):
    """presence, not value: also NAME=0 and NAME= (empty) turn a flag on, and nothing else moves"""
    for name in FLAGS:
        assert read_switches(**{name: value}) == dict(DEFAULTS, **{name: 1}), name


def test_numeric_switches_are_clamped_as_documented(read_switches):
    def one(name, value):
        return read_switches(**{name: value})
    assert one("NLE_STREAM64_CHUNK_MB", "0") == dict(DEFAULTS, NLE_STREAM64_CHUNK_MB=1)
    assert one("NLE_STREAM64_CHUNK_MB", "64") == dict(DEFAULTS, NLE_STREAM64_CHUNK_MB=64)
    assert one("NLE_SORTED_WGS_PER_CU", "0") == dict(DEFAULTS, NLE_SORTED_WGS_PER_CU=1)
    assert one("NLE_SORTED_WGS_PER_CU", "4") == dict(DEFAULTS, NLE_SORTED_WGS_PER_CU=4)
    assert one("NLE_DEV_SOLVER_MIN", "1") == dict(DEFAULTS, NLE_DEV_SOLVER_MIN=3)
    assert one("NLE_DEV_SOLVER_MIN", "64") == dict(DEFAULTS, NLE_DEV_SOLVER_MIN=64)
    # the number of workgroups is taken as given (0 and negatives included: the launcher then leaves it to the host solver);
    # unset is told apart from 0: the library's own choice for the order
    assert one("NLE_SYTRD_G", "250") == dict(DEFAULTS, sytrd_g_set=1, NLE_SYTRD_G=250)
    assert one("NLE_SYTRD_G", "0") == dict(DEFAULTS, sytrd_g_set=1, NLE_SYTRD_G=0)
    assert one("NLE_SYTRD_G", "-3") == dict(DEFAULTS, sytrd_g_set=1, NLE_SYTRD_G=-3)
    assert read_switches()["sytrd_g_set"] == 0


def test_q_solver_is_lanczos_or_nothing(read_switches):
    assert read_switches(NLE_Q_SOLVER="lanczos") == dict(DEFAULTS, NLE_Q_SOLVER=1)
    for other in ("", "1", "Lanczos", "lanczos ", "full"):
        assert read_switches(NLE_Q_SOLVER=other) == DEFAULTS, other
