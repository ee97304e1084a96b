"""Python mirror of the C ABI in include/nle.h (ctypes; no compute happens in Python).

The product is `lib/libnle_hip.so` (HIP kernels for gfx950 + host pipeline).  This module
only binds it for tests and `bench.py`, using torch tensors as device memory and the
torch current stream as the HIP stream -- plumbing, not the product.  There is no CPU
fallback: every compute call needs the shared library and a HIP device and raises
otherwise.  Nothing here imports `oracle/`.

Names follow the reference (`include/filter.hpp:20-54`): `NLEFilter.train_filter`
<-> `NLEFilter::trainFilter`, `.apply` <-> `::apply`, `transform_eigenvalues`
<-> `transformEigenValues`, `eigen_decomposition` <-> `eigenDecomposition`, ...
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnle_hip.so")

# the signature table and the integer constants are generated from include/nle.h (tools/gen_ctypes.py -> _abi.py;
# tests/test_abi.py regenerates and compares), so this mirror cannot drift from the header
from . import _abi
from ._abi import (ALLREDUCE_FN, NLE_ERR_COMM, NLE_ERR_HIP, NLE_ERR_INVALID, NLE_ERR_NUMERIC, NLE_OK)  # noqa: F401

EPS = 1e-10  # NLE_EPS
KERNEL_COUNT = _abi.NLE_KERNEL_COUNT
_P = C.c_void_p
_SIGNATURES = _abi.SIGNATURES
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
MODE_AUTO, MODE_MATERIALISED, MODE_PHI_FREE, MODE_PHI_FREE_EXP, MODE_MATERIALISED_F64, MODE_STREAMED_F64 = (
    _abi.NLE_MODE_AUTO, _abi.NLE_MODE_MATERIALISED, _abi.NLE_MODE_PHI_FREE, _abi.NLE_MODE_PHI_FREE_EXP,
    _abi.NLE_MODE_MATERIALISED_F64, _abi.NLE_MODE_STREAMED_F64)
MODE_EXACT_F64 = _abi.NLE_MODE_EXACT_F64  # the exact (Nystrom-free) filter, opt-in
EXACT_MAX_PIXELS = _abi.NLE_EXACT_MAX_PIXELS
SAMPLER_GRID, SAMPLER_FARTHEST = _abi.NLE_SAMPLER_GRID, _abi.NLE_SAMPLER_FARTHEST
SAMPLER_RESIDUAL = _abi.NLE_SAMPLER_RESIDUAL
# region edits: the bounds and the output kinds of nle_region_combine / nle_apply_regions
REGION_MAX, REGION_LAYERS_MAX = _abi.NLE_REGION_MAX, _abi.NLE_REGION_LAYERS_MAX
REGION_OUT_F32, REGION_OUT_ROUNDED8, REGION_OUT_U8 = (_abi.NLE_REGION_OUT_F32, _abi.NLE_REGION_OUT_ROUNDED8,
                                                      _abi.NLE_REGION_OUT_U8)
DETAIL_GAIN_MAX = _abi.NLE_DETAIL_GAIN_MAX  # nle_detail_combine / nle_apply_detail: the gain lies in [0, DETAIL_GAIN_MAX]
PLANES_MAX = _abi.NLE_PLANES_MAX  # nle_apply_planes: planes per call (its output kinds are REGION_OUT_F32 / _ROUNDED8)
RESID_AUTO, RESID_ROWS, RESID_FUSED = _abi.NLE_RESID_AUTO, _abi.NLE_RESID_ROWS, _abi.NLE_RESID_FUSED  # nle_nystrom_residual
# the MSE-guided denoiser: nle_nlm8's limits, the pre-filters of the denoise wrapper, every timed kernel id (KERNEL_COUNT
# stays the count of the train / apply path's ids)
NLM_PATCH_RADIUS_MAX, NLM_SEARCH_RADIUS_MAX = _abi.NLE_NLM_PATCH_RADIUS_MAX, _abi.NLE_NLM_SEARCH_RADIUS_MAX
PREFILTER_BILATERAL, PREFILTER_NLM = _abi.NLE_PREFILTER_BILATERAL, _abi.NLE_PREFILTER_NLM
KERNEL_COUNT_ALL = _abi.NLE_KERNEL_COUNT_ALL
# the base tone curve: the knots of a curve (a curve is [lo, hi, T_0 .. T_N]: TONE_KNOTS + 2 values), the histogram's bins
# (its counts: underflow, the bins, overflow and NaN: TONE_BINS + 2 values)
TONE_KNOTS, TONE_BINS = _abi.NLE_TONE_KNOTS, _abi.NLE_TONE_BINS
REGION_WEIGHT_ONE = _abi.NLE_REGION_WEIGHT_ONE  # nle_region_histograms: the count of one pixel with membership 1
LOCAL_SATURATION_MAX = _abi.NLE_LOCAL_SATURATION_MAX  # nle_local_chroma: a row's saturation lies in [0, LOCAL_SATURATION_MAX]
SEGMENT_ITERATIONS_MAX = _abi.NLE_SEGMENT_ITERATIONS_MAX  # nle_filter_segment: the cap on its iterations (C: 1 .. REGION_MAX)

_lib = None


class NLEError(RuntimeError):
    """Non-zero status from the C ABI (the C++ surface maps these to std::runtime_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def lib() -> C.CDLL:
    """Load libnle_hip.so (built by build.py).  Fails loudly if it is missing."""
    global _lib
    if _lib is None:
        # NLE_LIB_PATH: a measurement build of the same sources (tools/abl_run.sh) instead of the product library -- so that
        # such a build never has to be copied over lib/libnle_hip.so
        path = os.environ.get("NLE_LIB_PATH") or LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: run `python nonlocal-image-edit_amd/build.py` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        # torch-rocm ships its own copy of the HIP runtime: load torch first so that this process ends up
        # with ONE libamdhip64 (loading ours first leaves torch and the library on different runtimes and
        # hipGetDeviceCount then reports no device)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _check(status: int, ctx=None):
    if status != NLE_OK:
        msg = lib().nle_last_error(ctx)
        raise NLEError(status, (msg or b"").decode() or f"nle status {status}")


# ------------------------------------------------------------------ host-only helpers
def ld(n: int) -> int:
    return int(lib().nle_ld(int(n)))


def rccl_unique_id() -> bytes:
    buf = (C.c_char * 128)()
    _check(lib().nle_rccl_unique_id(buf, 128))
    return bytes(buf)


def lab8_tables():
    """tables of the fixed-point 8-bit BGR -> Lab conversion (nle_lab8_tables): gamma[256], cbrt[3072], coeffs[3][3]"""
    g = np.zeros(256, dtype=np.uint16)
    c = np.zeros(3072, dtype=np.uint16)
    k = np.zeros(9, dtype=np.int32)
    _check(lib().nle_lab8_tables(_np_ptr(g), _np_ptr(c), _np_ptr(k)))
    return g, c, k.reshape(3, 3)


def lab8_inverse_tables():
    """tables of the integer 8-bit Lab -> BGR conversion (nle_lab8_inverse_tables): yf[256][2], ab_to_xz[36864] (index
    t + 8145), inv_gamma[4096], coeffs[3][3] (rows R, G, B)"""
    yf = np.zeros(512, dtype=np.uint16)
    ab = np.zeros(36864, dtype=np.int32)
    ig = np.zeros(4096, dtype=np.uint16)
    k = np.zeros(9, dtype=np.int32)
    _check(lib().nle_lab8_inverse_tables(_np_ptr(yf), _np_ptr(ab), _np_ptr(ig), _np_ptr(k)))
    return yf.reshape(256, 2), ab, ig, k.reshape(3, 3)


def srgb16_tables():
    """tables of the 16-bit sRGB <-> float Lab conversion (nle_srgb16_tables): lin[65536], thr[65536] (thr[0] = -inf),
    forward[3][3] (rows X, Y, Z; columns R, G, B), inverse[3][3] (rows R, G, B; columns X, Y, Z), all float64"""
    lin = np.zeros(65536, dtype=np.float64)
    thr = np.zeros(65536, dtype=np.float64)
    k = np.zeros(18, dtype=np.float64)
    _check(lib().nle_srgb16_tables(_np_ptr(lin), _np_ptr(thr), _np_ptr(k)))
    return lin, thr, k[:9].reshape(3, 3).copy(), k[9:].reshape(3, 3).copy()


def sample_grid(H, W, n_row_samples, n_col_samples):
    """`samplePixels` (src/filter.cpp:56-80) in closed form.
    Returns dict(row_step,row_off,n_sel_rows,col_step,col_off,n_sel_cols)."""
    out = [C.c_int() for _ in range(6)]
    st = lib().nle_sample_grid(H, W, n_row_samples, n_col_samples, *[C.byref(o) for o in out])
    if st != NLE_OK:
        raise NLEError(st, "Number of samples per row and col must be <= that of image.")
    keys = ("row_step", "row_off", "n_sel_rows", "col_step", "col_off", "n_sel_cols")
    return dict(zip(keys, (o.value for o in out)))


def table_workspace(n_sel_rows, n_sel_cols, nrows, gram=False):
    """doubles of workspace of Context.table_pass (or table_gram) for nrows local rows (nle_table_workspace); -1 beyond 32 x 36"""
    return int(lib().nle_table_workspace(int(n_sel_rows), int(n_sel_cols), int(nrows), int(bool(gram))))


def residual_sampler_bytes(H, W, n_row_samples, n_col_samples):
    """device bytes SAMPLER_RESIDUAL's factor takes on an H x W plane with this sample grid (nle_residual_sampler_bytes);
    -1 for a grid sample_grid refuses"""
    return int(lib().nle_residual_sampler_bytes(int(H), int(W), int(n_row_samples), int(n_col_samples)))


def slab_rows(H, rank, world):
    r0, r1 = C.c_int(), C.c_int()
    st = lib().nle_slab_rows(H, rank, world, C.byref(r0), C.byref(r1))
    if st != NLE_OK:
        raise NLEError(st, "bad slab arguments")
    return r0.value, r1.value


def eigen_decomposition(M: np.ndarray, eps: float = EPS):
    """`eigenDecomposition` (src/filter.cpp:204-228): returns (U, D), descending, cut at eps."""
    M = np.asfortranarray(np.asarray(M, dtype=np.float64))
    n = M.shape[0]
    if M.ndim != 2 or M.shape[1] != n or n == 0:
        raise NLEError(NLE_ERR_INVALID, "eigen_decomposition needs a non-empty square matrix")
    U = np.zeros((n, n), dtype=np.float64, order="F")
    D = np.zeros(n, dtype=np.float64)
    r = C.c_int()
    st = lib().nle_eigen_decomposition(_np_ptr(M), n, float(eps), _np_ptr(U), _np_ptr(D), C.byref(r))
    if st != NLE_OK:
        raise NLEError(st, "eigensolver did not converge")
    return np.ascontiguousarray(U[:, :r.value]), D[:r.value].copy()


def eigen_decomposition_top(M: np.ndarray, kmax: int, eps: float = EPS):
    """all eigenvalues (descending) and the first min(kmax, n) eigenvectors: (U [n x min(kmax, n)], D [n], r)"""
    M = np.asfortranarray(np.asarray(M, dtype=np.float64))
    n = M.shape[0]
    k = min(int(kmax), n)
    U = np.zeros((n, k), dtype=np.float64, order="F")
    D = np.zeros(n, dtype=np.float64)
    r = C.c_int()
    st = lib().nle_eigen_decomposition_top(_np_ptr(M), n, float(eps), int(kmax), _np_ptr(U), _np_ptr(D), C.byref(r))
    if st != NLE_OK:
        raise NLEError(st, "eigensolver did not converge")
    return np.ascontiguousarray(U), D, r.value


def eigen_decomposition_topk(M: np.ndarray, kmax: int, eps: float = EPS):
    """the min(kmax, n) largest eigenvalues (descending), their eigenvectors and the number of eigenvalues >= eps, as the
    train path computes them for Q on the host (bisection when 2 kmax <= n): (U [n x k], Dk [k], r)"""
    M = np.asfortranarray(np.asarray(M, dtype=np.float64))
    n = M.shape[0]
    k = min(int(kmax), n)
    U = np.zeros((n, k), dtype=np.float64, order="F")
    D = np.zeros(k, dtype=np.float64)
    r = C.c_int()
    st = lib().nle_eigen_decomposition_topk(_np_ptr(M), n, float(eps), int(kmax), _np_ptr(U), _np_ptr(D), C.byref(r))
    if st != NLE_OK:
        raise NLEError(st, "eigensolver did not converge")
    return np.ascontiguousarray(U), D, r.value


def topk_eigen_decomposition(M: np.ndarray, n_largest: int, eps: float = EPS):
    """`topkEigenDecomposition` (src/filter.cpp:170-199, the USE_SPECTRA build): Lanczos top-k; returns (U, D)."""
    M = np.asfortranarray(np.asarray(M, dtype=np.float64))
    n = M.shape[0]
    nev = min(int(n_largest), n - 1)
    U = np.zeros((n, nev), dtype=np.float64, order="F")
    D = np.zeros(nev, dtype=np.float64)
    r = C.c_int()
    st = lib().nle_topk_eigen_decomposition(_np_ptr(M), n, int(n_largest), float(eps), _np_ptr(U), _np_ptr(D), C.byref(r))
    if st != NLE_OK:
        raise NLEError(st, "Lanczos did not converge")
    return np.ascontiguousarray(U[:, :r.value]), D[:r.value].copy()


def transform_eigenvalues(eigvals, weights):
    """`transformEigenValues` (src/filter.cpp:334-347)."""
    ev = np.ascontiguousarray(eigvals, dtype=np.float64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    out = np.zeros_like(ev)
    st = lib().nle_transform_eigenvalues(_np_ptr(ev), ev.size, _np_ptr(w), w.size, _np_ptr(out))
    if st != NLE_OK:
        raise NLEError(st, "bad arguments")
    return out


def layer_responses(eigvals, n_layers):
    ev = np.ascontiguousarray(eigvals, dtype=np.float64)
    out = np.zeros((n_layers, ev.size), dtype=np.float64)
    st = lib().nle_layer_responses(_np_ptr(ev), ev.size, n_layers, _np_ptr(out))
    if st != NLE_OK:
        raise NLEError(st, "bad arguments")
    return out


# ------------------------------------------------------------------ device side
def mse_shrink(eigvals, b, sigma, k_max, n_grid=256):
    """nle_mse_shrink (host only): (k, mse) -- the power k on the grid k_max i / n_grid that minimises the estimated MSE of the
    shrinkage min(max(lambda, 0), 1)^k for coefficients b under noise sigma, and the n_grid + 1 MSE values"""
    ev = np.ascontiguousarray(eigvals, dtype=np.float64).ravel()
    bb = np.ascontiguousarray(b, dtype=np.float64).ravel()
    if bb.size != ev.size:
        raise NLEError(NLE_ERR_INVALID, f"one coefficient per eigenvalue expected: {ev.size} eigenvalues, {bb.size} coefficients")
    n_grid = int(n_grid)
    mse = np.zeros(max(n_grid, 0) + 1)
    k = C.c_double(0.0)
    st = lib().nle_mse_shrink(_np_ptr(ev), _np_ptr(bb), ev.size, float(sigma), float(k_max), n_grid, C.byref(k), _np_ptr(mse))
    if st != NLE_OK:
        raise NLEError(st, "nle_mse_shrink: K >= 1, 1 <= n_grid <= 65536, sigma and k_max finite and >= 0 expected")
    return k.value, mse


def tone_curve(counts, shadows=0.0, highlights=0.0, clip_percent=-1.0, equalise=0.0):
    """nle_tone_curve (host only): the TONE_KNOTS + 2 values [lo, hi, T_0 .. T_N] of the base tone curve from the TONE_BINS + 2
    counts of Context.plane_histogram; counts may be None when clip_percent < 0 and equalise == 0"""
    cp = None
    if counts is not None:
        cnt = np.ascontiguousarray(counts, dtype=np.int64).ravel()
        if cnt.size != TONE_BINS + 2:
            raise NLEError(NLE_ERR_INVALID, f"tone_curve: {TONE_BINS + 2} counts expected, got {cnt.size}")
        cp = _np_ptr(cnt)
    curve = np.zeros(TONE_KNOTS + 2)
    _check(lib().nle_tone_curve(cp, float(shadows), float(highlights), float(clip_percent), float(equalise), _np_ptr(curve)))
    return curve


def _curve_ptr(curve, who):
    c = np.ascontiguousarray(curve, dtype=np.float64).ravel()
    if c.size != TONE_KNOTS + 2:
        raise NLEError(NLE_ERR_INVALID, f"{who}: a curve holds {TONE_KNOTS + 2} values [lo, hi, T_0 .. T_N], got {c.size}")
    return c


def _local_rows(who, M, L, weights, detail, curves):
    """the per-row arguments of nle_local_combine / nle_apply_local as contiguous arrays: weights (M + 1, L); detail
    (M + 1, 3) = (w_rho, gain, sigma) per row, None: (0, 1, 0) for every row; curves: None, or M + 1 entries, each None (no
    base curve for that row) or a curve [lo, hi, T_0 .. T_N].  Returns (w, d, on, cv) with on / cv None where no curve is on."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (M + 1, L):
        raise NLEError(NLE_ERR_INVALID, f"{who}: weights must be {(M + 1, L)}, got {w.shape}")
    d = np.tile([0.0, 1.0, 0.0], (M + 1, 1)) if detail is None else np.ascontiguousarray(detail, dtype=np.float64)
    if d.shape != (M + 1, 3):
        raise NLEError(NLE_ERR_INVALID, f"{who}: detail must be {(M + 1, 3)} (w_rho, gain, sigma per row), got {d.shape}")
    if curves is None or all(c is None for c in curves):
        return w, d, None, None
    if len(curves) != M + 1:
        raise NLEError(NLE_ERR_INVALID, f"{who}: curves must hold M + 1 = {M + 1} entries, got {len(curves)}")
    on = np.array([c is not None for c in curves], dtype=np.int32)
    cv = np.zeros((M + 1, TONE_KNOTS + 2))
    for m, c in enumerate(curves):
        if c is not None:
            cv[m] = _curve_ptr(c, who)
    return w, d, on, cv


def _combine_out(out, n, out_kind, device):
    """the output of a pointwise combine: `out` if given, else n float32 values, or n bytes for REGION_OUT_U8"""
    if out is not None:
        return out
    torch = _torch()
    return torch.empty(n, dtype=torch.uint8 if out_kind == REGION_OUT_U8 else torch.float32, device=device)


def _torch():
    import torch
    return torch


class Context:
    """`nle_ctx`: one per process/GPU.  Uses torch's current stream on `device`."""

    def __init__(self, device: int = 0, rank: int = 0, world: int = 1, allreduce=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device: nonlocal-image-edit_amd has no CPU fallback")
        self.device = int(device)
        torch.cuda.set_device(self.device)
        self._h = C.c_void_p()
        self._pinned = []
        # A dedicated torch stream: its handle is never the null stream (a NULL stream argument means
        # "create your own" in the C ABI), torch collectives issued under it are ordered with the
        # kernels of the ctx, and `_sync_in` orders the ctx after whatever produced its inputs.
        self._stream = torch.cuda.Stream(device=self.device)
        st = lib().nle_ctx_create(self.device, C.c_void_p(self._stream.cuda_stream), C.byref(self._h))
        if st != NLE_OK:
            raise NLEError(st, (lib().nle_last_error(None) or b"").decode())
        self.rank, self.world = rank, world
        self.slab_input = False
        self._cb = None
        self._comm = None
        self._allreduce = allreduce
        self._chroma = None  # set_chroma: the a and b planes the ctx borrows

    def set_shard(self, rank: int, world: int, n_samples: int, allreduce):
        """`allreduce(tensor)` sums a float64 CUDA tensor in place over all ranks (e.g.
        torch.distributed.all_reduce)."""
        torch = _torch()
        n = int(lib().nle_comm_len(int(n_samples)))
        self._comm = torch.zeros(n, dtype=torch.float64, device=f"cuda:{self.device}")
        comm = self._comm
        base = comm.data_ptr()

        debug_path = os.environ.get("NLE_DEBUG_COMM")
        views = {}   # (offset, count) -> tensor view: the Sinkhorn loop calls this 2T times with the same slice
        stream_ctx = torch.cuda.stream

        def _cb(user, d_buf, count):
            try:
                key = (int(d_buf), int(count))
                view = views.get(key)
                if view is None:
                    off = (key[0] - base) // 8
                    view = views[key] = comm[off:off + key[1]]
                if debug_path:
                    with open(debug_path + f".rank{rank}", "a") as fh:
                        fh.write(f"{key[1]}\n")
                with stream_ctx(self._stream):   # same stream as the ctx's kernels
                    allreduce(view)
                return 0
            except Exception as e:  # noqa: BLE001 - must not propagate through C
                print("nle allreduce callback failed:", repr(e), flush=True)
                return 1

        self._cb = ALLREDUCE_FN(_cb)
        _check(lib().nle_ctx_set_shard(self._h, rank, world, self._cb, None, C.c_void_p(base), n), self._h)
        self.rank, self.world = rank, world

    def init_rccl(self, rank: int, world: int, unique_id: bytes):
        """native RCCL all-reduces (nle_ctx_init_rccl): collective over the `world` ranks; `unique_id` = the 128 bytes of
        rccl_unique_id() made by rank 0"""
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        _check(lib().nle_ctx_init_rccl(self._h, int(rank), int(world), buf, 128), self._h)
        self.rank, self.world = rank, world

    def abort_rccl(self):
        """nle_ctx_abort_rccl: the error path of a multi-rank host (collectives of this ctx fail from here on)"""
        _check(lib().nle_ctx_abort_rccl(self._h))

    def synchronize(self):
        _check(lib().nle_ctx_synchronize(self._h), self._h)

    def set_mode(self, mode: int):
        """0 auto, 1 materialised Phi, 2 Phi-free, ..., 6 the exact filter (NLE_MODE_* in include/nle.h)."""
        _check(lib().nle_ctx_set_mode(self._h, int(mode)), self._h)

    def set_patch_radius(self, radius: int):
        """patch (non-local-means) affinities over (2R + 1)^2 neighbourhoods, 0 <= R <= NLE_PATCH_RADIUS_MAX; 0 (default) is
        the reference's single-value affinity (nle_ctx_set_patch_radius)"""
        _check(lib().nle_ctx_set_patch_radius(self._h, int(radius)), self._h)

    def set_chroma(self, a=None, b=None, hc: float = 0.0):
        """chroma-aware (Lab) affinities: the a and b planes of 8-bit Lab (H x W, integer valued in [0, 255]) and the chroma
        bandwidth hc > 0; a = b = None turns them off (nle_ctx_set_chroma).  The ctx borrows the planes: the device
        tensors made here are kept alive until they are replaced or cleared."""
        if a is None and b is None:
            _check(lib().nle_ctx_set_chroma(self._h, None, None, float(hc)), self._h)
            self._chroma = None
            return
        ta = None if a is None else self._lum(a)
        tb = None if b is None else self._lum(b)
        _torch().cuda.synchronize(self.device)  # the planes are complete before any later train reads them
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _check(lib().nle_ctx_set_chroma(self._h, ptr(ta), ptr(tb), float(hc)), self._h)
        self._chroma = (ta, tb)

    def set_sampler(self, sampler: int):
        """sample selection: SAMPLER_GRID (0, default, the reference's grid), SAMPLER_FARTHEST (1, farthest-point
        selection in the affinity's metric) or SAMPLER_RESIDUAL (3, residual-greedy: pivoted Cholesky on the affinity;
        nle_ctx_set_sampler)"""
        _check(lib().nle_ctx_set_sampler(self._h, int(sampler)), self._h)

    def sample_pixels(self, lum, n_row_samples, n_col_samples, hx, hy):
        """the ctx's sample set on the full plane `lum` (nle_sample_pixels): row-major pixel indices, ascending, int64"""
        x = self._lum(lum)
        H, W = x.shape
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        out = np.zeros(g["n_sel_rows"] * g["n_sel_cols"], dtype=np.int64)
        p = C.c_int()
        _check(lib().nle_sample_pixels(self._h, C.c_void_p(x.data_ptr()), H, W, int(n_row_samples), int(n_col_samples),
                                       float(hx), float(hy), _np_ptr(out), C.byref(p)), self._h)
        return out[:p.value]

    def sample_pixels_order(self, lum, n_row_samples, n_col_samples, hx, hy):
        """SAMPLER_RESIDUAL's selection on the full plane `lum` as it was made (nle_sample_pixels_order): dict(order [int64,
        the samples in the order chosen], pivot [float64: d of the sample when chosen, after the fallback its farthest-point
        m], n_residual, stats [max d over the pixels not chosen, its first index, sum max(d, 0) after the last residual
        round])"""
        x = self._lum(lum)
        H, W = x.shape
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        n = g["n_sel_rows"] * g["n_sel_cols"]
        order, pivot, stats = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64), np.zeros(3, dtype=np.float64)
        p, nres = C.c_int(), C.c_int()
        _check(lib().nle_sample_pixels_order(self._h, C.c_void_p(x.data_ptr()), H, W, int(n_row_samples), int(n_col_samples),
                                             float(hx), float(hy), _np_ptr(order), _np_ptr(pivot), C.byref(p), C.byref(nres),
                                             _np_ptr(stats)), self._h)
        return dict(order=order[:p.value], pivot=pivot[:p.value], n_residual=nres.value, stats=stats)

    def nystrom_residual(self, lum, n_row_samples, n_col_samples, hx, hy, form: int = RESID_AUTO, thresh: float = 0.5,
                         want_map: bool = True):
        """the Nystrom residual map r_i = 1 - k_i^T pinv(K_A) k_i of the full plane `lum` under the ctx's affinity options
        (nle_nystrom_residual): returns (r [H x W float32 CUDA tensor, or None without want_map], summary) with summary =
        dict(sum, max, argmax (row-major index of the first maximum), count (pixels with r > thresh))"""
        torch = _torch()
        x = self._lum(lum)
        H, W = x.shape
        r = torch.empty((H, W), dtype=torch.float32, device=x.device) if want_map else None
        self._sync_in()
        s = np.zeros(4, dtype=np.float64)
        _check(lib().nle_nystrom_residual(self._h, C.c_void_p(x.data_ptr()), H, W, int(n_row_samples), int(n_col_samples),
                                          float(hx), float(hy), int(form), float(thresh),
                                          C.c_void_p(r.data_ptr()) if want_map else None, _np_ptr(s)), self._h)
        return r, dict(sum=float(s[0]), max=float(s[1]), argmax=int(s[2]), count=int(s[3]))

    def affinity_product64(self, lum, X, hx, hy):
        """Y = K X with K the exact N x N affinity of the H x W plane `lum` (integer valued in [0, 255]; the kernel of
        MODE_EXACT_F64, nle_affinity_product64).  X: N x ncols (or N) float64, numpy or CUDA; returns an N x ncols float64
        CUDA tensor."""
        torch = _torch()
        lum = self._lum(lum)
        H, W = lum.shape
        X = torch.as_tensor(X, dtype=torch.float64, device=lum.device)
        if X.ndim == 1:
            X = X[:, None]
        N, ncols = X.shape
        if N != H * W:
            raise NLEError(NLE_ERR_INVALID, f"X must have H * W = {H * W} rows, got {N}")
        ldx = ld(ncols)
        Xp = torch.zeros((N, ldx), dtype=torch.float64, device=lum.device)
        Xp[:, :ncols] = X
        Y = torch.empty_like(Xp)
        self._sync_in()
        _check(lib().nle_affinity_product64(self._h, C.c_void_p(lum.data_ptr()), H, W, float(hx), float(hy),
                                            C.c_void_p(Xp.data_ptr()), ldx, ncols, C.c_void_p(Y.data_ptr())), self._h)
        return Y[:, :ncols]

    def set_train_reduce(self, on: bool = True):
        """trains leave apply's reduce half for their own plane and applies may take it over (nle_ctx_set_train_reduce)"""
        _check(lib().nle_ctx_set_train_reduce(self._h, 1 if on else 0), self._h)

    def set_nystrom_bf16x3(self, on: bool = True):
        """the fused Nystrom GEMM on the bf16 matrix cores with split operands (nle_ctx_set_nystrom_bf16x3)"""
        _check(lib().nle_ctx_set_nystrom_bf16x3(self._h, 1 if on else 0), self._h)

    def host_alloc(self, shape, dtype=np.float32):
        """page-locked host array (nle_host_alloc).  The block belongs to the ctx and is freed by Context.close(): the
        returned array (and every view of it) must not be used after that"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        _check(lib().nle_host_alloc(self._h, n, C.byref(ptr)), self._h)
        buf = (C.c_char * max(n, 1)).from_address(ptr.value)
        self._pinned.append(ptr)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def eigen_decomposition_top_device(self, M, kmax: int, eps: float = EPS):
        """eigen_decomposition_top with the tridiagonal reduction on the GPU (nle_eigen_decomposition_top_device; n <= 224)"""
        M = np.asfortranarray(np.asarray(M, dtype=np.float64))
        n = M.shape[0]
        k = min(int(kmax), n)
        U = np.zeros((n, k), dtype=np.float64, order="F")
        D = np.zeros(n, dtype=np.float64)
        r = C.c_int()
        _check(lib().nle_eigen_decomposition_top_device(self._h, _np_ptr(M), n, float(eps), int(kmax), _np_ptr(U), _np_ptr(D),
                                                        C.byref(r)), self._h)
        return np.ascontiguousarray(U), D, r.value

    def sym_eigen_device(self, M, first: int = 0, count: int = 0, eps: float = EPS):
        """all eigenvalues (descending) and the eigenvectors of D[first:first+count] with the reduction, the bisection and the
        back-transformation on the GPU (nle_sym_eigen_device; 3 <= n <= 1152).  Returns (U n x count, D, r)."""
        M = np.asfortranarray(np.asarray(M, dtype=np.float64))
        n = M.shape[0]
        U = np.zeros((n, max(count, 1)), dtype=np.float64, order="F")
        D = np.zeros(n, dtype=np.float64)
        r = C.c_int()
        _check(lib().nle_sym_eigen_device(self._h, _np_ptr(M), n, float(eps), int(first), int(count), _np_ptr(U), _np_ptr(D),
                                          C.byref(r)), self._h)
        return np.ascontiguousarray(U[:, :count]), D, r.value

    def cholesky_device(self, M, out=None):
        """(L, L^-1, trace(M^-1), ok) of a symmetric matrix (lower triangle read) on the GPU (nle_cholesky_device).
        out = (L, Linv): caller's n x n float64 buffers (flat or 2-D, e.g. page-locked from host_alloc), filled
        COLUMN-major and returned as they are"""
        M = np.asfortranarray(np.asarray(M, dtype=np.float64))
        n = M.shape[0]
        if out is None:
            L = np.zeros((n, n), dtype=np.float64, order="F")
            Li = np.zeros((n, n), dtype=np.float64, order="F")
        else:
            L, Li = out
            if any(a.dtype != np.float64 or a.size != n * n for a in (L, Li)):
                raise NLEError(NLE_ERR_INVALID, "cholesky_device: out buffers must hold n * n float64 values")
        tr = C.c_double()
        ok = C.c_int()
        _check(lib().nle_cholesky_device(self._h, _np_ptr(M), n, _np_ptr(L), _np_ptr(Li), C.byref(tr), C.byref(ok)), self._h)
        if out is not None:
            return L, Li, tr.value, bool(ok.value)
        return np.ascontiguousarray(L), np.ascontiguousarray(Li), tr.value, bool(ok.value)

    def set_slab_input(self, on: bool = True):
        """planes passed to train / apply hold this rank's rows only (nle_ctx_set_slab_input); pass shape=(H, W)"""
        _check(lib().nle_ctx_set_slab_input(self._h, 1 if on else 0), self._h)
        self.slab_input = bool(on)

    def set_topk_solver(self, solver: int):
        """0: full eigensolve of Q (the reference's default build); 1: Lanczos top-K (its USE_SPECTRA build)"""
        _check(lib().nle_ctx_set_topk_solver(self._h, int(solver)), self._h)

    def trim(self):
        """release the cached device workspace"""
        _check(lib().nle_ctx_trim(self._h), self._h)

    def profile(self, enable=True):
        """Per-kernel HIP-event timing on the ctx's stream (resets the counters).  True / 2: every
        kernel; 1: the N-sized kernels only (cheaper: each timed launch costs ~10 us of stream gaps)."""
        level = 2 if enable is True else int(enable)
        _check(lib().nle_ctx_profile(self._h, level), self._h)

    def kernel_stats(self):
        """{kernel name: (launches, total_ms)} accumulated since `profile(True)`."""
        out = {}
        for kid in range(KERNEL_COUNT_ALL):
            n, ms = C.c_longlong(), C.c_double()
            _check(lib().nle_ctx_kernel_stats(self._h, kid, C.byref(n), C.byref(ms)), self._h)
            out[lib().nle_kernel_name(kid).decode()] = (n.value, ms.value)
        return out

    def close(self):
        if self._h:
            for ptr in self._pinned:
                lib().nle_host_free(self._h, ptr)
            self._pinned = []
            lib().nle_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _sync_in(self):
        """order the ctx stream after the work already queued on torch's current stream"""
        torch = _torch()
        self._stream.wait_stream(torch.cuda.current_stream(self.device))

    # ---- stage-level entry points (device tensors in/out) ----
    def _lum(self, lum):
        torch = _torch()
        t = torch.as_tensor(lum, dtype=torch.float32, device=f"cuda:{self.device}").contiguous()
        if t.ndim != 2:
            raise NLEError(NLE_ERR_INVALID, "luminance must be H x W")
        self._sync_in()
        return t

    def local_pixels(self, H, W):
        r0, r1 = slab_rows(H, self.rank, self.world)
        return (r1 - r0) * W

    def compute_kernel(self, lum, n_row_samples, n_col_samples, hx, hy, want_kab=True):
        """`computeKernel` (src/filter.cpp:114-167): returns (Ka [p x p fp64 numpy],
        kab [n_local x ld(p) fp32 CUDA tensor, natural pixel order])."""
        torch = _torch()
        lum = self._lum(lum)
        H, W = lum.shape
        if n_row_samples > H or n_col_samples > W:
            raise NLEError(NLE_ERR_INVALID, "Number of samples per row and col must be <= that of image.")
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        Ka = np.zeros((p, p), dtype=np.float64, order="F")
        kab = None
        if want_kab:
            kab = torch.empty((self.local_pixels(H, W), ld(p)), dtype=torch.float32, device=lum.device)
        _check(lib().nle_compute_kernel(self._h, C.c_void_p(lum.data_ptr()), H, W, n_row_samples, n_col_samples,
                                        float(hx), float(hy), _np_ptr(Ka),
                                        C.c_void_p(kab.data_ptr()) if want_kab else None), self._h)
        return np.ascontiguousarray(Ka), kab

    def nystrom(self, lum, n_row_samples, n_col_samples, hx, hy):
        """`nystromApproximation` fused with the affinity evaluation: (eigvals, phi[n_local x ld(r)])."""
        torch = _torch()
        lum = self._lum(lum)
        H, W = lum.shape
        if n_row_samples > H or n_col_samples > W:
            raise NLEError(NLE_ERR_INVALID, "Number of samples per row and col must be <= that of image.")
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        n_local = self.local_pixels(H, W)
        buf = torch.empty(n_local * ld(p), dtype=torch.float32, device=lum.device)
        ev = np.zeros(p, dtype=np.float64)
        r = C.c_int()
        _check(lib().nle_nystrom(self._h, C.c_void_p(lum.data_ptr()), H, W, n_row_samples, n_col_samples, float(hx),
                                 float(hy), _np_ptr(ev), C.byref(r), C.c_void_p(buf.data_ptr())), self._h)
        rr = r.value
        return ev[:rr].copy(), buf[: n_local * ld(rr)].view(n_local, ld(rr)), rr

    def ts_gemm(self, A, kd, B):
        """C = A[:, :kd] @ B  (A fp32 CUDA M x lda, B fp64 numpy kd x nc) -> CUDA M x ld(nc)."""
        torch = _torch()
        self._sync_in()
        B = np.asfortranarray(np.asarray(B, dtype=np.float64))
        M, lda = A.shape
        nc = B.shape[1]
        Cc = torch.empty((M, ld(nc)), dtype=torch.float32, device=A.device)
        _check(lib().nle_ts_gemm(self._h, C.c_void_p(A.data_ptr()), M, lda, kd, _np_ptr(B), nc,
                                 C.c_void_p(Cc.data_ptr())), self._h)
        return Cc

    def sinkhorn_scalings(self, phi, r, eigvals, max_iter=10):
        """Sinkhorn iterations (src/filter.cpp:238-245) on device phi -> (u_c, u_r)."""
        ev = np.ascontiguousarray(eigvals, dtype=np.float64)
        uc, ur = np.zeros(r), np.zeros(r)
        self._sync_in()
        M, ldp = phi.shape
        _check(lib().nle_sinkhorn_scalings(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(ev), max_iter,
                                           _np_ptr(uc), _np_ptr(ur)), self._h)
        return uc, ur

    def gram(self, phi, r, u=None):
        """sum_i c_i^2 phi_i phi_i^T (r x r), c_i = recip(phi_i . u); u None: c_i = 1 (nle_gram's h_u == NULL)"""
        self._sync_in()
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.size < r:
                raise NLEError(NLE_ERR_INVALID, "gram: need r entries of u")
        G = np.zeros((r, r), dtype=np.float64, order="F")
        M, ldp = phi.shape
        _check(lib().nle_gram(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(u) if u is not None else None,
                              _np_ptr(G)), self._h)
        return np.ascontiguousarray(G)

    def row_scalings(self, phi, r, u):
        torch = _torch()
        self._sync_in()
        u = np.ascontiguousarray(u, dtype=np.float64)
        M, ldp = phi.shape
        out = torch.empty(M, dtype=torch.float64, device=phi.device)
        _check(lib().nle_row_scalings(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(u),
                                      C.c_void_p(out.data_ptr())), self._h)
        return out

    # the same stages on fp64 device matrices (nle_*64): X is a float64 CUDA tensor (M, ld), rows contiguous (a row
    # sub-block X[q:] included), ANY ld >= the logical width; columns >= the logical width are never read
    def _mat64(self, X, width, what):
        torch = _torch()
        if X.dtype != torch.float64 or X.ndim != 2 or not X.is_cuda:
            raise NLEError(NLE_ERR_INVALID, f"{what}: need a float64 device tensor (M, ld)")
        M, ldx = X.shape
        if X.stride(1) != 1 or (M > 1 and X.stride(0) != ldx):
            raise NLEError(NLE_ERR_INVALID, f"{what}: rows must be contiguous with stride ld")
        if not 1 <= width <= ldx:
            raise NLEError(NLE_ERR_INVALID, f"{what}: need 1 <= logical width <= ld")
        self._sync_in()
        return M, ldx

    def ts_gemm64(self, A, kd, B):
        """C = A[:, :kd] @ B  (A fp64 CUDA M x lda, B fp64 numpy kd x nc) -> fp64 CUDA M x ld(nc)."""
        torch = _torch()
        M, lda = self._mat64(A, kd, "ts_gemm64")
        B = np.asfortranarray(np.asarray(B, dtype=np.float64))
        if B.ndim != 2 or B.shape[0] != kd:
            raise NLEError(NLE_ERR_INVALID, "ts_gemm64: B must be kd x nc")
        nc = B.shape[1]
        Cc = torch.empty((M, ld(nc)), dtype=torch.float64, device=A.device)
        _check(lib().nle_ts_gemm64(self._h, C.c_void_p(A.data_ptr()), M, lda, kd, _np_ptr(B), nc,
                                   C.c_void_p(Cc.data_ptr())), self._h)
        return Cc

    def sinkhorn_scalings64(self, phi, r, eigvals, max_iter=10):
        """Sinkhorn iterations (src/filter.cpp:238-245) on fp64 device phi -> (u_c, u_r); r <= 2048."""
        M, ldp = self._mat64(phi, r, "sinkhorn_scalings64")
        ev = np.ascontiguousarray(eigvals, dtype=np.float64)
        if ev.size < r:
            raise NLEError(NLE_ERR_INVALID, "sinkhorn_scalings64: need r eigenvalues")
        uc, ur = np.zeros(r), np.zeros(r)
        _check(lib().nle_sinkhorn_scalings64(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(ev), max_iter,
                                             _np_ptr(uc), _np_ptr(ur)), self._h)
        return uc, ur

    def gram64(self, phi, r, u=None):
        """sum_i c_i^2 phi_i phi_i^T (r x r), c_i = recip(phi_i . u); u None: c_i = 1"""
        M, ldp = self._mat64(phi, r, "gram64")
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.size < r:
                raise NLEError(NLE_ERR_INVALID, "gram64: need r entries of u")
        G = np.zeros((r, r), dtype=np.float64, order="F")
        _check(lib().nle_gram64(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(u) if u is not None else None,
                                _np_ptr(G)), self._h)
        return np.ascontiguousarray(G)

    def row_scalings64(self, phi, r, u):
        torch = _torch()
        M, ldp = self._mat64(phi, r, "row_scalings64")
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.size < r:
            raise NLEError(NLE_ERR_INVALID, "row_scalings64: need r entries of u")
        out = torch.empty(M, dtype=torch.float64, device=phi.device)
        _check(lib().nle_row_scalings64(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, _np_ptr(u),
                                        C.c_void_p(out.data_ptr())), self._h)
        return out

    # ---- the sample-space stages (csrc/fused.hip), each alone: nle_sample_pass / _gram / _project / _update ----
    def _plane(self, lum):
        torch = _torch()
        t = torch.as_tensor(lum, dtype=torch.float32, device=f"cuda:{self.device}").contiguous()
        self._sync_in()
        return t, int(t.shape[0]), int(t.shape[1])

    def sample_pass(self, lum, nr, nc, hx, hy, w=None, recip=False, rows=None, want_y=True):
        """one Sinkhorn half-iteration over rows [row0, row1) of the plane: (z (p), y (M, device) or None)"""
        torch = _torch()
        t, H, W = self._plane(lum)
        row0, row1 = rows if rows is not None else (0, H)
        g = sample_grid(H, W, nr, nc)
        z = np.zeros(g["n_sel_rows"] * g["n_sel_cols"])
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        if w is not None and w.size != z.size:
            raise NLEError(NLE_ERR_INVALID, "sample_pass: need p entries of w")
        y = torch.empty(max(row1 - row0, 0) * W, dtype=torch.float64, device=t.device) if want_y else None
        _check(lib().nle_sample_pass(self._h, C.c_void_p(t.data_ptr()), H, W, nr, nc, hx, hy, row0, row1, int(bool(recip)),
                                     _np_ptr(w) if w is not None else None, C.c_void_p(y.data_ptr()) if want_y else None,
                                     _np_ptr(z)), self._h)
        return z, y

    def sample_gram(self, lum, nr, nc, hx, hy, c, rows=None):
        """sum over the non-sample pixels of rows [row0, row1) of c_i^2 k_i k_i^T (p x p); c: M doubles on the device"""
        t, H, W = self._plane(lum)
        row0, row1 = rows if rows is not None else (0, H)
        if c.dtype != _torch().float64 or not c.is_cuda or c.numel() != (row1 - row0) * W or not c.is_contiguous():
            raise NLEError(NLE_ERR_INVALID, "sample_gram: c must be M float64 values on the device")
        g = sample_grid(H, W, nr, nc)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        G = np.zeros((p, p))
        _check(lib().nle_sample_gram(self._h, C.c_void_p(t.data_ptr()), H, W, nr, nc, hx, hy, row0, row1,
                                     C.c_void_p(c.data_ptr()), _np_ptr(G)), self._h)
        return G

    def sample_project(self, lum, nr, nc, hx, hy, D, c, rows=None, out=None):
        """V (M x ld(K) fp32, device) = diag(c) K_rows D over rows [row0, row1); D: p x K, c: M doubles on the device.
        out: an (M, ld(K)) float32 device tensor to write into (whatever it holds)"""
        torch = _torch()
        t, H, W = self._plane(lum)
        row0, row1 = rows if rows is not None else (0, H)
        D = np.ascontiguousarray(D, dtype=np.float64)
        g = sample_grid(H, W, nr, nc)
        if D.ndim != 2 or D.shape[0] != g["n_sel_rows"] * g["n_sel_cols"]:
            raise NLEError(NLE_ERR_INVALID, "sample_project: D must be p x K")
        K, M = D.shape[1], (row1 - row0) * W
        if c.dtype != torch.float64 or not c.is_cuda or c.numel() != M or not c.is_contiguous():
            raise NLEError(NLE_ERR_INVALID, "sample_project: c must be M float64 values on the device")
        ldv = (K + 3) & ~3
        V = out if out is not None else torch.empty((M, ldv), dtype=torch.float32, device=t.device)
        if V.dtype != torch.float32 or tuple(V.shape) != (M, ldv) or not V.is_contiguous() or not V.is_cuda:
            raise NLEError(NLE_ERR_INVALID, "sample_project: out must be an (M, ld(K)) float32 device tensor")
        _check(lib().nle_sample_project(self._h, C.c_void_p(t.data_ptr()), H, W, nr, nc, hx, hy, row0, row1, _np_ptr(D), K,
                                        C.c_void_p(c.data_ptr()), C.c_void_p(V.data_ptr()), ldv), self._h)
        return V

    def sample_update(self, X1, X2, lam, z, sA=None, chol=False):
        """the p-sized update between two passes on host operands.  X1, X2: (2p, r) arrays (the library takes the first
        column-major, the second row-major), z: (zrows, zld) slices, sA None: the column sum -> (v (2p), u (r), sA_next, w_next)"""
        X = np.asarray(X1, dtype=np.float64)
        X1c, X2r = np.asfortranarray(X), np.ascontiguousarray(np.asarray(X2, dtype=np.float64))
        n2, r = X.shape
        p = n2 // 2
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        z = np.ascontiguousarray(np.atleast_2d(z), dtype=np.float64)
        sA = None if sA is None else np.ascontiguousarray(sA, dtype=np.float64)
        if n2 != 2 * p or X2r.shape != (n2, r) or lam.size != r or z.shape[1] < p or (sA is not None and sA.size != p):
            raise NLEError(NLE_ERR_INVALID, "sample_update: X1, X2 (2p x r), lam (r), z (zrows x zld >= p), sA (p)")
        v, u, sn, wn = np.zeros(n2), np.zeros(r), np.zeros(p), np.zeros(p)
        self._sync_in()
        _check(lib().nle_sample_update(self._h, p, r, int(bool(chol)), int(sA is not None), _np_ptr(X1c), _np_ptr(X2r),
                                       _np_ptr(lam), _np_ptr(z), z.shape[0], z.shape[1], _np_ptr(sA) if sA is not None else None,
                                       _np_ptr(v), _np_ptr(u), _np_ptr(sn), _np_ptr(wn)), self._h)
        return v, u, sn, wn

    # ---- the table path's stages (csrc/tables.hip), each alone: nle_table_* ----
    def _dev64(self, a, what, n=None):
        """`a` (array or tensor, or None) as a contiguous float64 device tensor of n entries"""
        if a is None:
            return None
        torch = _torch()
        t = torch.as_tensor(a, dtype=torch.float64, device=f"cuda:{self.device}").contiguous()
        if n is not None and t.numel() != n:
            raise NLEError(NLE_ERR_INVALID, f"{what}: need {n} doubles, got {t.numel()}")
        return t

    def _table_view(self, lum, nr, nc, rows, tables, hx, hy, c, who):
        """the arguments every nle_table_* call that takes a view starts with, and (tensors to keep alive, grid, row0, nrows)"""
        t, H, W = self._plane(lum)
        row0, row1 = rows if rows is not None else (0, H)
        g = sample_grid(H, W, nr, nc)
        nR, nC, nrows = g["n_sel_rows"], g["n_sel_cols"], max(row1 - row0, 0)
        keep = [t]
        if tables is not None:
            er, ecT, Ep = (self._dev64(a, who, n) for a, n in zip(tables, (nrows * nR, nC * W, 256 * nR * nC)))
            keep += [er, ecT, Ep]
        cv = self._dev64(c, who, nrows * W)
        keep.append(cv)
        self._sync_in()
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        args = [self._h, ptr(t), H, W, int(nr), int(nc), int(row0), int(row1), float(hx), float(hy)]
        args += [ptr(a) for a in (keep[1:4] if tables is not None else (None, None, None))] + [ptr(cv)]
        return args, keep, dict(g, H=H, W=W, row0=row0, nrows=nrows, p=nR * nC, ldp=(nR * nC + 63) & ~63)

    def table_levels(self, x):
        """check_levels over the float32 device tensor `x` (a view at any element offset): (bad, 16-bit tile mask)"""
        if x.dtype != _torch().float32 or not x.is_cuda or not x.is_contiguous():
            raise NLEError(NLE_ERR_INVALID, "table_levels: x must be contiguous float32 values on the device")
        self._sync_in()
        bad, mask = C.c_int(-1), C.c_uint(0)
        _check(lib().nle_table_levels(self._h, C.c_void_p(x.data_ptr()), x.numel(), C.byref(bad), C.byref(mask)), self._h)
        return bad.value, mask.value

    def table_build(self, lum, nr, nc, hx, hy, rows=None, tables=None):
        """what the view is (nle_table_build): dict(sorted, lev_t0, lev_nt, index_sums, layers_per_launch, er, ecT, Ep)"""
        torch = _torch()
        args, keep, g = self._table_view(lum, nr, nc, rows, tables, hx, hy, None, "table_build")
        dev = keep[0].device
        er = torch.empty((g["nrows"], g["n_sel_rows"]), dtype=torch.float64, device=dev)
        ecT = torch.empty((g["n_sel_cols"], g["W"]), dtype=torch.float64, device=dev)
        Ep = torch.empty((256, g["p"]), dtype=torch.float64, device=dev)
        info = (C.c_int * 5)()
        _check(lib().nle_table_build(*args, C.c_void_p(er.data_ptr()), C.c_void_p(ecT.data_ptr()), C.c_void_p(Ep.data_ptr()), info),
               self._h)
        return dict(sorted=bool(info[0]), lev_t0=info[1], lev_nt=info[2], index_sums=bool(info[3]), layers_per_launch=info[4],
                    er=er, ecT=ecT, Ep=Ep)

    def table_pass(self, lum, nr, nc, mode, rows=None, tables=None, hx=0.0, hy=0.0, c=None, w=None, x=None):
        """one half-iteration of the table pass (nle_table_pass; mode 0 column sum, 1 reciprocal with w, 2 y = c x with the
        full plane x): dict(z (ldp), y (nrows W), ws (the whole workspace: g, h, the partial rows), n (nrows nC 256))"""
        torch = _torch()
        args, keep, g = self._table_view(lum, nr, nc, rows, tables, hx, hy, c, "table_pass")
        dev = keep[0].device
        wv = self._dev64(w, "table_pass: w", g["p"])
        xv = None if x is None else torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
        if xv is not None and xv.numel() != g["H"] * g["W"]:
            raise NLEError(NLE_ERR_INVALID, "table_pass: x is the full H x W plane")
        n_ws = int(lib().nle_table_workspace(g["n_sel_rows"], g["n_sel_cols"], max(g["nrows"], 1), 0))
        ws = torch.empty(max(n_ws, 1), dtype=torch.float64, device=dev)
        z = torch.empty(g["ldp"], dtype=torch.float64, device=dev)
        y = torch.empty(g["nrows"] * g["W"], dtype=torch.float64, device=dev)
        self._sync_in()
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
        _check(lib().nle_table_pass(*args, int(mode), ptr(wv), ptr(xv), ptr(y), ptr(ws), ws.numel(), ptr(z)), self._h)
        return dict(z=z, y=y, ws=ws, n=g["nrows"] * g["n_sel_cols"] * 256)

    def table_expand(self, lum, nr, nc, wl, c, rows=None, tables=None, hx=0.0, hy=0.0, round8=False, ostride=None):
        """the expand half of apply for the nl weight vectors wl (nl x ldw): (g tables (nl, nrows, nC, 256), planes (nl, ostride))"""
        torch = _torch()
        args, keep, g = self._table_view(lum, nr, nc, rows, tables, hx, hy, c, "table_expand")
        dev = keep[0].device
        wl = torch.as_tensor(wl, dtype=torch.float64, device=dev).contiguous()
        if wl.ndim != 2:
            raise NLEError(NLE_ERR_INVALID, "table_expand: wl must be nl x ldw")
        nl, ldw = int(wl.shape[0]), int(wl.shape[1])
        ostride = g["nrows"] * g["W"] if ostride is None else int(ostride)
        gws = torch.empty((nl, g["nrows"], g["n_sel_cols"], 256), dtype=torch.float64, device=dev)
        out = torch.empty((nl, ostride), dtype=torch.float32, device=dev)
        self._sync_in()
        _check(lib().nle_table_expand(*args, C.c_void_p(wl.data_ptr()), ldw, nl, int(bool(round8)), C.c_void_p(gws.data_ptr()),
                                      C.c_void_p(out.data_ptr()), ostride), self._h)
        return gws, out

    def table_gram(self, lum, nr, nc, c, rows=None, tables=None, hx=0.0, hy=0.0):
        """sum over the non-sample pixels of rows [row0, row1) of c_i^2 k_i k_i^T through the tables: (Gk (p, p), workspace,
        (rows per GEMM split, number of splits))"""
        torch = _torch()
        args, keep, g = self._table_view(lum, nr, nc, rows, tables, hx, hy, c, "table_gram")
        dev = keep[0].device
        n_ws = int(lib().nle_table_workspace(g["n_sel_rows"], g["n_sel_cols"], max(g["nrows"], 1), 1))
        ws = torch.empty(max(n_ws, 1), dtype=torch.float64, device=dev)
        Gk = torch.empty((g["p"], g["p"]), dtype=torch.float64, device=dev)
        self._sync_in()
        split = (C.c_int * 2)()
        _check(lib().nle_table_gram(*args, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(Gk.data_ptr()), split), self._h)
        return Gk, ws, (split[0], split[1])

    def table_apply_small(self, m, D, Vrows, xA, resp, ldw, differs=None, m_same=None, xA_same=None):
        """the p- and K-sized middle of apply on host operands.  D, Vrows: (p, ldk) with K = resp.shape[1] <= ldk logical
        columns, resp: (L, K), differs: None, 0 or 1 -> (t (K), W' (L, ldw), YA (L, p))"""
        torch = _torch()
        D = np.ascontiguousarray(D, dtype=np.float64)
        resp = np.ascontiguousarray(np.atleast_2d(resp), dtype=np.float64)
        (p, ldk), (L, K) = D.shape, resp.shape
        dev = f"cuda:{self.device}"
        d = {k: self._dev64(v, "table_apply_small") for k, v in dict(m=m, D=D, V=Vrows, xA=xA, resp=resp, ms=m_same, xs=xA_same).items()}
        flag = None if differs is None else torch.tensor([int(differs)], dtype=torch.int32, device=dev)
        t = torch.empty(max(K, 1), dtype=torch.float64, device=dev)
        Wp = torch.empty((L, max(int(ldw), 1)), dtype=torch.float64, device=dev)
        YA = torch.empty((L, p), dtype=torch.float64, device=dev)
        self._sync_in()
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
        _check(lib().nle_table_apply_small(self._h, p, K, ldk, L, int(ldw), ptr(d["m"]), ptr(d["D"]), ptr(d["V"]), ptr(d["xA"]),
                                           ptr(d["resp"]), ptr(t), ptr(Wp), ptr(YA), ptr(flag), ptr(d["ms"]), ptr(d["xs"])), self._h)
        return t.cpu().numpy()[:K], Wp.cpu().numpy(), YA.cpu().numpy()

    def table_scatter(self, loc, YA, Y, round8=False):
        """Y[l, loc[a]] = (float)YA[l, a] where loc[a] >= 0, in place in the (L, ystride) float32 device tensor Y"""
        torch = _torch()
        dev = f"cuda:{self.device}"
        YA = self._dev64(np.atleast_2d(YA), "table_scatter")
        L, p = int(YA.shape[0]), int(YA.shape[1])
        loc = torch.as_tensor(np.ascontiguousarray(loc, dtype=np.int64), device=dev)
        if Y.dtype != torch.float32 or not Y.is_cuda or not Y.is_contiguous() or Y.ndim != 2 or Y.shape[0] != L or loc.numel() != p:
            raise NLEError(NLE_ERR_INVALID, "table_scatter: Y must be an (L, ystride) float32 device tensor, loc p indices")
        self._sync_in()
        _check(lib().nle_table_scatter(self._h, p, L, C.c_void_p(loc.data_ptr()), C.c_void_p(YA.data_ptr()), C.c_void_p(Y.data_ptr()),
                                       int(Y.shape[1]), int(bool(round8))), self._h)
        return Y

    def gemm64s(self, m, n, kk, A, sA, B, sB, Cm, sC, dl=None, dk=None, dr=None, add=None, sadd=(0, 0)):
        """nle_gemm64s on float64 CUDA tensors, in place in Cm: A, B, Cm (and add) are taken as flat buffers whose entry
        (i, j) sits at i * s[0] + j * s[1] doubles from data_ptr(); dl, dk, dr: vectors or None"""
        self._sync_in()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _check(lib().nle_gemm64s(self._h, m, n, kk, ptr(A), sA[0], sA[1], ptr(B), sB[0], sB[1], ptr(Cm), sC[0], sC[1],
                                 ptr(dl), ptr(dk), ptr(dr), ptr(add), sadd[0], sadd[1]), self._h)
        return Cm

    # ---- colour / denoise wrapper pieces (device tensors) ----
    def bgr2lab8(self, bgr):
        """`cvtColor(COLOR_BGR2Lab)` on an H x W x 3 uint8 image: (lab uint8 H x W x 3, L float32 H x W)"""
        torch = _torch()
        t = torch.as_tensor(bgr, dtype=torch.uint8, device=f"cuda:{self.device}").contiguous()
        self._sync_in()
        H, W = t.shape[:2]
        lab = torch.empty_like(t)
        L = torch.empty((H, W), dtype=torch.float32, device=t.device)
        _check(lib().nle_bgr2lab8(self._h, C.c_void_p(t.data_ptr()), H * W, C.c_void_p(lab.data_ptr()),
                                  C.c_void_p(L.data_ptr())), self._h)
        return lab, L

    def lab8_channel(self, lab, channel):
        torch = _torch()
        self._sync_in()
        H, W = lab.shape[:2]
        out = torch.empty((H, W), dtype=torch.float32, device=lab.device)
        _check(lib().nle_lab8_channel(self._h, C.c_void_p(lab.data_ptr()), H * W, int(channel),
                                      C.c_void_p(out.data_ptr())), self._h)
        return out

    def lab2bgr8(self, lab, L=None, a=None, b=None):
        """`max/min/convertTo(CV_8U)/merge/cvtColor(COLOR_Lab2BGR)` with optional float32 replacement planes"""
        torch = _torch()
        self._sync_in()
        H, W = lab.shape[:2]
        out = torch.empty_like(lab)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _check(lib().nle_lab2bgr8_planes(self._h, C.c_void_p(lab.data_ptr()), ptr(L), ptr(a), ptr(b), H * W,
                                         C.c_void_p(out.data_ptr())), self._h)
        return out

    # ---- deep colour: 16-bit sRGB <-> float Lab (device tensors; 16-bit images as torch.uint16) ----
    def _u16(self, bgr):
        """an (..., 3) 16-bit BGR image on the device, contiguous (numpy uint16 or a torch.uint16 tensor)"""
        torch = _torch()
        if isinstance(bgr, np.ndarray):
            bgr = torch.from_numpy(np.array(bgr, dtype=np.uint16, order="C"))  # a copy: the caller's array may be read-only
        if bgr.dtype != torch.uint16 or bgr.shape[-1] != 3:
            raise NLEError(NLE_ERR_INVALID, "a 16-bit image is (..., 3) uint16 in B, G, R order")
        return bgr.to(f"cuda:{self.device}").contiguous()

    def bgr16_to_lab(self, bgr, want_ab=True, want_guide=True):
        """nle_bgr16_to_lab on an (..., 3) uint16 BGR image: (L, a, b, guide) float32 planes of the image's leading shape,
        a and b None without want_ab, guide None without want_guide"""
        torch = _torch()
        t = self._u16(bgr)
        self._sync_in()
        shape, n = t.shape[:-1], t.numel() // 3
        new = lambda: torch.empty(shape, dtype=torch.float32, device=t.device)  # noqa: E731
        L, a, b, g = new(), (new() if want_ab else None), (new() if want_ab else None), (new() if want_guide else None)
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        _check(lib().nle_bgr16_to_lab(self._h, ptr(t), n, ptr(L), ptr(a), ptr(b), ptr(g)), self._h)
        return L, a, b, g

    def lab_to_bgr16(self, L, a, b):
        """nle_lab_to_bgr16 on float32 planes of one shape: the (..., 3) torch.uint16 BGR image"""
        torch = _torch()
        dev = f"cuda:{self.device}"
        L, a, b = (torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous() for x in (L, a, b))
        if a.shape != L.shape or b.shape != L.shape:
            raise NLEError(NLE_ERR_INVALID, "L, a and b must have one shape")
        self._sync_in()
        out = torch.empty(tuple(L.shape) + (3,), dtype=torch.uint16, device=L.device)
        _check(lib().nle_lab_to_bgr16(self._h, C.c_void_p(L.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                      L.numel(), C.c_void_p(out.data_ptr())), self._h)
        return out

    # ---- HDR tone mapping: linear-light float BGR -> log-luminance planes -> 16-bit sRGB (device tensors) ----
    def _f32bgr(self, bgr):
        """an (..., 3) linear-light float32 BGR image on the device, contiguous (numpy or torch)"""
        torch = _torch()
        if isinstance(bgr, np.ndarray) and bgr.dtype == np.float32:
            bgr = torch.from_numpy(np.array(bgr, order="C"))  # a copy: the caller's array may be read-only
        t = torch.as_tensor(bgr)
        if t.dtype != torch.float32 or t.dim() < 1 or t.shape[-1] != 3:
            raise NLEError(NLE_ERR_INVALID, "an HDR image is (..., 3) float32 in B, G, R order")
        return t.to(f"cuda:{self.device}").contiguous()

    def hdr_range(self, bgr):
        """nle_hdr_range on an (..., 3) float32 BGR image: (l_hi, range) as Python floats"""
        t = self._f32bgr(bgr)
        self._sync_in()
        l_hi, rng = C.c_double(0.0), C.c_double(0.0)
        _check(lib().nle_hdr_range(self._h, C.c_void_p(t.data_ptr()), t.numel() // 3, C.byref(l_hi), C.byref(rng)), self._h)
        return l_hi.value, rng.value

    def hdr_to_loglum(self, bgr, l_hi, rng, want_x=True, want_guide=True):
        """nle_hdr_to_loglum: (x, guide) float32 planes of the image's leading shape, None where not wanted"""
        torch = _torch()
        t = self._f32bgr(bgr)
        self._sync_in()
        shape = t.shape[:-1]
        x = torch.empty(shape, dtype=torch.float32, device=t.device) if want_x else None
        g = torch.empty(shape, dtype=torch.float32, device=t.device) if want_guide else None
        ptr = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
        _check(lib().nle_hdr_to_loglum(self._h, ptr(t), t.numel() // 3, float(l_hi), float(rng), ptr(x), ptr(g)), self._h)
        return x, g

    def loglum_to_bgr16(self, y, bgr, l_hi, rng, base_weight, saturation=1.0):
        """nle_loglum_to_bgr16 on the filtered plane y and the original (..., 3) float32 BGR image: the (..., 3) torch.uint16
        BGR image"""
        torch = _torch()
        t = self._f32bgr(bgr)
        y = torch.as_tensor(y, dtype=torch.float32, device=t.device).contiguous()
        if y.numel() != t.numel() // 3:
            raise NLEError(NLE_ERR_INVALID, "y must have one value per pixel of the image")
        self._sync_in()
        out = torch.empty(t.shape, dtype=torch.uint16, device=t.device)
        _check(lib().nle_loglum_to_bgr16(self._h, C.c_void_p(y.data_ptr()), C.c_void_p(t.data_ptr()), y.numel(), float(l_hi),
                                         float(rng), float(base_weight), float(saturation), C.c_void_p(out.data_ptr())), self._h)
        return out

    def bilateral8(self, plane, sigma_color, sigma_space):
        """`cv::bilateralFilter(plane, -1, sigmaColor, sigmaSpace)` on an integer-valued float32 plane"""
        torch = _torch()
        src = self._lum(plane)
        H, W = src.shape
        out = torch.empty_like(src)
        _check(lib().nle_bilateral8(self._h, C.c_void_p(src.data_ptr()), H, W, float(sigma_color), float(sigma_space),
                                    C.c_void_p(out.data_ptr())), self._h)
        return out

    def nlm8(self, plane, patch_radius, search_radius, sigma, h, want_raw=False):
        """nle_nlm8 on an integer-valued float32 plane: the rounded plane, or (rounded, raw) with want_raw"""
        torch = _torch()
        src = self._lum(plane)
        H, W = src.shape
        out = torch.empty_like(src)
        raw = torch.empty_like(src) if want_raw else None
        _check(lib().nle_nlm8(self._h, C.c_void_p(src.data_ptr()), H, W, int(patch_radius), int(search_radius), float(sigma),
                              float(h), C.c_void_p(out.data_ptr()), C.c_void_p(raw.data_ptr()) if want_raw else None), self._h)
        return (out, raw) if want_raw else out

    def plane_noise(self, plane):
        """nle_plane_noise on an integer-valued float32 plane: (S, sigma) -- Immerkaer's absolute sum (exact) and estimate"""
        src = self._lum(plane)
        H, W = src.shape
        S, sigma = C.c_longlong(0), C.c_double(0.0)
        _check(lib().nle_plane_noise(self._h, C.c_void_p(src.data_ptr()), H, W, C.byref(S), C.byref(sigma)), self._h)
        return S.value, sigma.value

    def region_combine(self, layers, q, weights, floor=0.05, out_kind=0, out=None):
        """nle_region_combine, the rule alone: layers (L, n) and q (M, n) float32 device tensors whose rows are contiguous
        and may lie any stride >= n apart (a view into a larger buffer, at any offset, is taken as it is); weights
        (M + 1, L) float64, row 0 the background.  Returns n float32 values, or n bytes for REGION_OUT_U8."""
        self._sync_in()
        L, n = layers.shape
        M = q.shape[0]
        if q.shape[1] != n or layers.stride(1) != 1 or q.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "region_combine: layers (L, n) and q (M, n) with contiguous rows")
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (M + 1, L):
            raise NLEError(NLE_ERR_INVALID, f"region_combine: weights must be {(M + 1, L)}, got {w.shape}")
        out = _combine_out(out, n, out_kind, layers.device)
        _check(lib().nle_region_combine(self._h, C.c_void_p(layers.data_ptr()), L, C.c_void_p(q.data_ptr()), M, n,
                                        layers.stride(0) if L > 1 else n, q.stride(0) if M > 1 else n, _np_ptr(w),
                                        float(floor), int(out_kind), C.c_void_p(out.data_ptr())), self._h)
        return out

    def detail_combine(self, x, layers, weights, residual_weight=0.0, gain=1.0, sigma=0.0, out_kind=0, out=None):
        """nle_detail_combine, the rule alone: x (n,) and layers (L, n) float32 device tensors, the rows of layers contiguous
        and any stride >= n apart (a view into a larger buffer, at any offset, is taken as it is); weights L float64 values.
        Returns n float32 values, or n bytes for REGION_OUT_U8."""
        self._sync_in()
        L, n = layers.shape
        if x.shape != (n,) or x.stride(0) != 1 or layers.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "detail_combine: x (n,) and layers (L, n) with contiguous rows")
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (L,):
            raise NLEError(NLE_ERR_INVALID, f"detail_combine: weights must hold L = {L} values, got {w.shape}")
        out = _combine_out(out, n, out_kind, layers.device)
        _check(lib().nle_detail_combine(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(layers.data_ptr()), L, n,
                                        layers.stride(0) if L > 1 else n, _np_ptr(w), float(residual_weight), float(gain),
                                        float(sigma), int(out_kind), C.c_void_p(out.data_ptr())), self._h)
        return out

    def plane_histogram(self, x, scale=1.0):
        """nle_plane_histogram: the TONE_BINS + 2 int64 counts of the float32 device values x (any shape, contiguous) times
        scale, in quarter levels over [-256, 768) between an underflow counter and one for overflow and NaN"""
        torch = _torch()
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=f"cuda:{self.device}")
        self._sync_in()
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise NLEError(NLE_ERR_INVALID, "plane_histogram: contiguous float32 values expected")
        counts = np.zeros(TONE_BINS + 2, dtype=np.int64)
        _check(lib().nle_plane_histogram(self._h, C.c_void_p(x.data_ptr()), x.numel(), float(scale), _np_ptr(counts)), self._h)
        return counts

    def tone_combine(self, x, layers, weights, curve, residual_weight=0.0, gain=1.0, sigma=0.0, out_kind=0, out=None):
        """nle_tone_combine, the rule alone: detail_combine with the base term w_{L-1} Y_{L-1} passed through `curve`
        ([lo, hi, T_0 .. T_N], what tone_curve returns).  Planes and result as for detail_combine."""
        self._sync_in()
        L, n = layers.shape
        if x.shape != (n,) or x.stride(0) != 1 or layers.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "tone_combine: x (n,) and layers (L, n) with contiguous rows")
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (L,):
            raise NLEError(NLE_ERR_INVALID, f"tone_combine: weights must hold L = {L} values, got {w.shape}")
        cv = _curve_ptr(curve, "tone_combine")
        out = _combine_out(out, n, out_kind, layers.device)
        _check(lib().nle_tone_combine(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(layers.data_ptr()), L, n,
                                      layers.stride(0) if L > 1 else n, _np_ptr(w), float(residual_weight), float(gain),
                                      float(sigma), _np_ptr(cv), int(out_kind), C.c_void_p(out.data_ptr())), self._h)
        return out

    def local_combine(self, x, layers, q, weights, detail=None, curves=None, floor=0.05, out_kind=0, out=None):
        """nle_local_combine, the rule alone: x (n,), layers (L, n) and q (M, n) float32 device tensors, rows contiguous and
        any stride >= n apart; weights (M + 1, L), row 0 the background; detail (M + 1, 3) = (w_rho, gain, sigma) per row
        (None: 0, 1, 0); curves: None, or M + 1 entries, each None or a curve of tone_curve for that row's base layer.
        Returns n float32 values, or n bytes for REGION_OUT_U8."""
        self._sync_in()
        L, n = layers.shape
        M = q.shape[0]
        if x.shape != (n,) or x.stride(0) != 1 or q.shape[1] != n or layers.stride(1) != 1 or q.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "local_combine: x (n,), layers (L, n) and q (M, n) with contiguous rows")
        w, d, on, cv = _local_rows("local_combine", M, L, weights, detail, curves)
        out = _combine_out(out, n, out_kind, layers.device)
        _check(lib().nle_local_combine(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(layers.data_ptr()), L,
                                       C.c_void_p(q.data_ptr()), M, n, layers.stride(0) if L > 1 else n,
                                       q.stride(0) if M > 1 else n, _np_ptr(w), _np_ptr(d), _np_ptr(on) if on is not None else None,
                                       _np_ptr(cv) if cv is not None else None, float(floor), int(out_kind),
                                       C.c_void_p(out.data_ptr())), self._h)
        return out

    def local_chroma(self, a, b, q, saturation, floor=0.05, out=None):
        """nle_local_chroma: a, b (n,) and q (M, n) float32 device tensors; saturation M + 1 values, row 0 the background.
        out: None (two new tensors), "inplace" (a and b are rewritten) or a pair of (n,) float32 tensors.  Returns (a', b')."""
        torch = _torch()
        self._sync_in()
        M, n = q.shape
        if a.shape != (n,) or b.shape != (n,) or a.stride(0) != 1 or b.stride(0) != 1 or q.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "local_chroma: a (n,), b (n,) and q (M, n) with contiguous rows")
        s = np.ascontiguousarray(saturation, dtype=np.float64)
        if s.shape != (M + 1,):
            raise NLEError(NLE_ERR_INVALID, f"local_chroma: saturation must hold M + 1 = {M + 1} values, got {s.shape}")
        ao, bo = (a, b) if isinstance(out, str) and out == "inplace" else out if out is not None else (torch.empty_like(a), torch.empty_like(b))
        _check(lib().nle_local_chroma(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(q.data_ptr()), M, n,
                                      q.stride(0) if M > 1 else n, _np_ptr(s), float(floor), C.c_void_p(ao.data_ptr()),
                                      C.c_void_p(bo.data_ptr())), self._h)
        return ao, bo

    def region_histograms(self, y, q, scale, row_on=None, floor=0.05):
        """nle_region_histograms: the membership-weighted histograms of y (n,) under the planes q (M, n), float32 device
        tensors with contiguous rows; scale M + 1 values, row 0 the background; row_on: None (every row) or M + 1 flags.
        Returns (M + 1, TONE_BINS + 2) int64 counts in units of 1 / REGION_WEIGHT_ONE of a pixel; rows that are off are zero."""
        self._sync_in()
        torch = _torch()
        if not (isinstance(y, torch.Tensor) and isinstance(q, torch.Tensor) and q.ndim == 2):
            raise NLEError(NLE_ERR_INVALID, "region_histograms: y (n,) and q (M, n) device tensors expected")
        M, n = q.shape
        if y.dtype != torch.float32 or q.dtype != torch.float32 or not self._here(y) or not self._here(q):
            raise NLEError(NLE_ERR_INVALID, "region_histograms: float32 tensors on this ctx's device expected")
        if y.shape != (n,) or y.stride(0) != 1 or q.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, "region_histograms: y (n,) and q (M, n) with contiguous rows")
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sc.shape != (M + 1,):
            raise NLEError(NLE_ERR_INVALID, f"region_histograms: scale must hold M + 1 = {M + 1} values, got {sc.shape}")
        on = None
        if row_on is not None:
            on = np.ascontiguousarray([1 if r else 0 for r in row_on], dtype=np.int32)
            if on.shape != (M + 1,):
                raise NLEError(NLE_ERR_INVALID, f"region_histograms: row_on must hold M + 1 = {M + 1} flags, got {on.shape}")
        counts = np.zeros((M + 1, TONE_BINS + 2), dtype=np.int64)
        _check(lib().nle_region_histograms(self._h, C.c_void_p(y.data_ptr()), C.c_void_p(q.data_ptr()), M, n,
                                           q.stride(0) if M > 1 else n, _np_ptr(sc), _np_ptr(on) if on is not None else None,
                                           float(floor), _np_ptr(counts)), self._h)
        return counts

    def _here(self, t):
        """t is a tensor on this ctx's device (its pointer is handed to kernels)"""
        return t.is_cuda and (t.device.index or 0) == self.device

    def _labels(self, labels, who, n):
        """the n labels as uint8 on this ctx's device: host values are uploaded, a device tensor is taken as it is"""
        torch = _torch()
        if not isinstance(labels, torch.Tensor):
            labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint8), device=f"cuda:{self.device}")
        if (labels.dtype != torch.uint8 or labels.ndim != 1 or labels.stride(0) != 1 or labels.numel() != n or
                not self._here(labels)):
            raise NLEError(NLE_ERR_INVALID, f"{who}: labels must be {n} contiguous bytes on cuda:{self.device} (a view at any "
                                            "offset is taken as it is)")
        return labels

    def _segment_planes(self, q, who):
        """(C, n) of float32 planes on this ctx's device with contiguous rows"""
        torch = _torch()
        if (not isinstance(q, torch.Tensor) or q.dtype != torch.float32 or q.ndim != 2 or q.stride(1) != 1 or
                not self._here(q)):
            raise NLEError(NLE_ERR_INVALID, f"{who}: (C, n) float32 planes on cuda:{self.device} with contiguous rows expected")
        return q.shape

    def segment_init(self, x, count):
        """nle_segment_init: the equal-population start of `count` clusters on the float32 device values x (any shape,
        contiguous; a view at any offset is taken as it is).  Returns (labels: n uint8 on the device, cuts: count - 1 ints)."""
        torch = _torch()
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=f"cuda:{self.device}")
        if x.dtype != torch.float32 or not x.is_contiguous() or not self._here(x):
            raise NLEError(NLE_ERR_INVALID, f"segment_init: contiguous float32 values on cuda:{self.device} expected")
        self._sync_in()
        labels = torch.zeros(x.numel(), dtype=torch.uint8, device=x.device)
        cuts = np.zeros(max(int(count) - 1, 1), dtype=np.int32)
        _check(lib().nle_segment_init(self._h, C.c_void_p(x.data_ptr()), x.numel(), int(count), C.c_void_p(labels.data_ptr()),
                                      _np_ptr(cuts)), self._h)
        return labels, cuts[:max(int(count) - 1, 0)]

    def segment_stats(self, q, labels):
        """nle_segment_stats: q (C, n) float32 device planes with contiguous rows any stride >= n apart (stride 0, an
        expanded plane, is taken as it is: every cluster then reads the one plane), labels n uint8.  Returns (counts int64,
        sums float64), C values each."""
        Cn, n = self._segment_planes(q, "segment_stats")
        labels = self._labels(labels, "segment_stats", n)
        self._sync_in()
        counts, sums = np.zeros(max(Cn, 1), dtype=np.int64), np.zeros(max(Cn, 1))
        _check(lib().nle_segment_stats(self._h, C.c_void_p(q.data_ptr()), Cn, n, q.stride(0) if Cn > 1 else n,
                                       C.c_void_p(labels.data_ptr()),
                                       _np_ptr(counts), _np_ptr(sums)), self._h)
        return counts[:Cn], sums[:Cn]

    def segment_assign(self, q, means, labels, want_indicators=False, indicators=None):
        """nle_segment_assign: q (C, n) as for segment_stats, means C float64 values (+inf: inactive), labels n uint8 on the
        device, REWRITTEN in place.  Returns (counts int64, changed), and the (C, n) float32 indicator planes of the new
        labels as a third value when want_indicators is set or `indicators` (rows contiguous, any stride >= n) is given."""
        torch = _torch()
        Cn, n = self._segment_planes(q, "segment_assign")
        labels = self._labels(labels, "segment_assign", n)
        m = np.ascontiguousarray(means, dtype=np.float64)
        if m.shape != (Cn,):
            raise NLEError(NLE_ERR_INVALID, f"segment_assign: {Cn} means expected, got {m.shape}")
        if indicators is None and want_indicators:
            indicators = torch.empty((Cn, n), dtype=torch.float32, device=q.device)
        if indicators is not None and tuple(self._segment_planes(indicators, "segment_assign (indicators)")) != (Cn, n):
            raise NLEError(NLE_ERR_INVALID, f"segment_assign: indicators must be float32 {(Cn, n)} with contiguous rows")
        self._sync_in()
        counts, changed = np.zeros(max(Cn, 1), dtype=np.int64), C.c_longlong(0)
        _check(lib().nle_segment_assign(self._h, C.c_void_p(q.data_ptr()), Cn, n, q.stride(0) if Cn > 1 else n, _np_ptr(m),
                                        C.c_void_p(labels.data_ptr()),
                                        C.c_void_p(indicators.data_ptr()) if indicators is not None else None,
                                        (indicators.stride(0) if Cn > 1 else n) if indicators is not None else 0,
                                        _np_ptr(counts), C.byref(changed)), self._h)
        return (counts[:Cn], changed.value) if indicators is None else (counts[:Cn], changed.value, indicators)

    def bench_affinity(self, lum, n_row_samples, n_col_samples, hx, hy, reps=10):
        torch = _torch()
        lum = self._lum(lum)
        H, W = lum.shape
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        kab = torch.empty((self.local_pixels(H, W), ld(p)), dtype=torch.float32, device=lum.device)
        ms = C.c_double()
        _check(lib().nle_bench_affinity(self._h, C.c_void_p(lum.data_ptr()), H, W, n_row_samples, n_col_samples,
                                        float(hx), float(hy), C.c_void_p(kab.data_ptr()), reps, C.byref(ms)), self._h)
        return ms.value, kab

    def bench_affinity64(self, lum, n_row_samples, n_col_samples, hx, hy, rows, reps=10):
        """average launch time (ms) of the fp64 affinity kernel on the first `rows` image rows; returns (ms, bytes written)"""
        torch = _torch()
        lum = self._lum(lum)
        H, W = lum.shape
        g = sample_grid(H, W, n_row_samples, n_col_samples)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        rows = int(min(rows, H))
        kab = torch.empty((rows * W, ld(p)), dtype=torch.float64, device=lum.device)
        ms = C.c_double()
        _check(lib().nle_bench_affinity64(self._h, C.c_void_p(lum.data_ptr()), H, W, n_row_samples, n_col_samples,
                                          float(hx), float(hy), rows, C.c_void_p(kab.data_ptr()), reps, C.byref(ms)), self._h)
        return ms.value, kab.numel() * 8

    def bench_sinkhorn_pass(self, phi, r, reps=10):
        self._sync_in()
        ms = C.c_double()
        M, ldp = phi.shape
        _check(lib().nle_bench_sinkhorn_pass(self._h, C.c_void_p(phi.data_ptr()), M, ldp, r, reps, C.byref(ms)),
               self._h)
        return ms.value


class NLEFilter:
    """`nle::NLEFilter` (include/filter.hpp:35-54) over the C ABI; state = V, eigvals on the GPU."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._f = C.c_void_p()
        self.shape = None
        self._train_plane = None

    def close(self):
        if self._f:
            lib().nle_filter_destroy(self._f)
            self._f = C.c_void_p()
        self._train_plane = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _full_shape(self, plane, shape):
        """(H, W) of the full image for a plane handed in: the plane's own shape, or -- Context.set_slab_input -- the
        `shape` given, the plane then being this rank's rows [row0, row1) (nle_slab_rows)"""
        if not getattr(self.ctx, "slab_input", False) or self.ctx.world == 1:
            return tuple(int(v) for v in plane.shape)
        if shape is None:
            raise NLEError(NLE_ERR_INVALID, "slab input: pass shape=(H, W) of the full image")
        H, W = int(shape[0]), int(shape[1])
        r0, r1 = slab_rows(H, self.ctx.rank, self.ctx.world)
        if tuple(plane.shape) != (r1 - r0, W):
            raise NLEError(NLE_ERR_INVALID, f"slab input: rank {self.ctx.rank} of {self.ctx.world} must pass rows "
                                            f"[{r0}, {r1}) x {W}, got {tuple(plane.shape)}")
        return H, W

    def train_filter(self, lum, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter=10, n_eigen_vectors=5, shape=None):
        """`NLEFilter::trainFilter` (src/filter.cpp:480-502); lum: H x W luminance (CUDA tensor
        stays on the device; numpy is uploaded).  Slab-input contexts pass their rows and shape=(H, W)."""
        self.close()
        lum = self.ctx._lum(lum)
        H, W = self._full_shape(lum, shape)
        _check(lib().nle_train(self.ctx._h, C.c_void_p(lum.data_ptr()), H, W, int(n_row_samples), int(n_col_samples),
                               float(hx), float(hy), int(n_sinkhorn_iter), int(n_eigen_vectors), C.byref(self._f)),
               self.ctx._h)
        self.shape = (H, W)
        self._train_plane = lum if self.ctx.world == 1 else None  # the start of segment()
        return self

    def train_filter_host(self, lum, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter=10, n_eigen_vectors=5,
                          shape=None):
        """nle_train_host: the H x W fp32 plane is a HOST array (pinned: Context.host_alloc); the filter keeps the
        uploaded plane for apply_layers_host(None, ...).  Slab-input contexts pass their rows and shape=(H, W)."""
        self.close()
        lum = np.ascontiguousarray(lum, dtype=np.float32)
        H, W = self._full_shape(lum, shape)
        _check(lib().nle_train_host(self.ctx._h, _np_ptr(lum), H, W, int(n_row_samples), int(n_col_samples), float(hx),
                                    float(hy), int(n_sinkhorn_iter), int(n_eigen_vectors), C.byref(self._f)), self.ctx._h)
        self.shape = (H, W)
        return self

    def train_filter_host_u8(self, lum8, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter=10, n_eigen_vectors=5,
                             shape=None):
        """nle_train_host_u8: the plane as the 8-bit levels themselves (a HOST uint8 array): a quarter of the upload; the
        same filter as train_filter_host on those levels as floats"""
        self.close()
        lum8 = np.ascontiguousarray(lum8, dtype=np.uint8)
        H, W = self._full_shape(lum8, shape)
        _check(lib().nle_train_host_u8(self.ctx._h, _np_ptr(lum8), H, W, int(n_row_samples), int(n_col_samples), float(hx),
                                       float(hy), int(n_sinkhorn_iter), int(n_eigen_vectors), C.byref(self._f)), self.ctx._h)
        self.shape = (H, W)
        return self

    def apply_layers_host(self, x, n_layers, out):
        """nle_apply_layers_host: x a HOST H x W fp32 array or None (= the training plane kept by
        train_filter_host); out: HOST (L, n_local) fp32 array"""
        H, W = self.shape
        n_local = self.info()["n_local"]
        xp = None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            want = n_local if (self.ctx.slab_input and self.ctx.world > 1) else H * W
            if x.size != want:
                raise NLEError(NLE_ERR_INVALID, f"apply_layers_host: x has {x.size} values, the filter needs {want}")
            xp = _np_ptr(x)
        # the library writes n_layers * n_local floats into `out`: a short array would be a host heap overflow
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous
                and out.size == int(n_layers) * n_local):
            raise NLEError(NLE_ERR_INVALID, f"apply_layers_host: out must be a C-contiguous float32 array of "
                                            f"{int(n_layers)} x {n_local} values")
        _check(lib().nle_apply_layers_host(self._f, xp, H, W, int(n_layers), _np_ptr(out)), self.ctx._h)
        return out

    def level_tiles(self):
        """(first, count) of the 16-level tiles the table kernels of this filter work on (nle_filter_level_tiles)"""
        a, b = C.c_int(), C.c_int()
        _check(lib().nle_filter_level_tiles(self._f, C.byref(a), C.byref(b)), self.ctx._h)
        return a.value, b.value

    def apply_u8_host(self, x, f_s, out):
        """nle_apply_u8_host: the 8-bit L plane `enhance` merges back (src/filter.cpp:428-436) -- apply, clamp to
        [0, 255], round half to even.  x a HOST H x W fp32 array or None (= the training plane); out: HOST uint8 array of
        n_local values"""
        H, W = self.shape
        n_local = self.info()["n_local"]
        fs = np.ascontiguousarray(f_s, dtype=np.float64)
        if fs.ndim != 1 or fs.size != self.info()["K"]:
            raise NLEError(NLE_ERR_INVALID, f"f_s must hold K' = {self.info()['K']} values, got {fs.shape}")
        xp = None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            want = n_local if (self.ctx.slab_input and self.ctx.world > 1) else H * W
            if x.size != want:
                raise NLEError(NLE_ERR_INVALID, f"apply_u8_host: x has {x.size} values, the filter needs {want}")
            xp = _np_ptr(x)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size == n_local):
            raise NLEError(NLE_ERR_INVALID, f"apply_u8_host: out must be a C-contiguous uint8 array of {n_local} values")
        _check(lib().nle_apply_u8_host(self._f, xp, H, W, _np_ptr(fs), _np_ptr(out)), self.ctx._h)
        return out

    def apply_rounded8(self, x, f_s, out=None):
        """nle_apply_rounded8: the clamped, rounded plane as fp32 levels (the replacement-channel argument of lab2bgr8)"""
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = self._full_shape(x, self.shape)
        fs = np.ascontiguousarray(f_s, dtype=np.float64)
        if fs.ndim != 1 or fs.size != self.info()["K"]:
            raise NLEError(NLE_ERR_INVALID, f"f_s must hold K' = {self.info()['K']} values, got {fs.shape}")
        n = self.info()["n_local"]
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=x.device)
        _check(lib().nle_apply_rounded8(self._f, C.c_void_p(x.data_ptr()), H, W, _np_ptr(fs), C.c_void_p(out.data_ptr())),
               self.ctx._h)
        return out

    def apply_u8(self, x, f_s, out=None):
        """nle_apply_u8: the same on a device-resident plane; returns a uint8 device tensor of n_local values"""
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = self._full_shape(x, self.shape)
        fs = np.ascontiguousarray(f_s, dtype=np.float64)
        if fs.ndim != 1 or fs.size != self.info()["K"]:
            raise NLEError(NLE_ERR_INVALID, f"f_s must hold K' = {self.info()['K']} values, got {fs.shape}")
        n = self.info()["n_local"]
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=x.device)
        _check(lib().nle_apply_u8(self._f, C.c_void_p(x.data_ptr()), H, W, _np_ptr(fs), C.c_void_p(out.data_ptr())),
               self.ctx._h)
        return out

    def info(self):
        n = C.c_longlong()
        v = [C.c_int() for _ in range(5)]
        _check(lib().nle_filter_info(self._f, C.byref(n), *[C.byref(x) for x in v]))
        return dict(n_local=n.value, K=v[0].value, r=v[1].value, p=v[2].value, row0=v[3].value, row1=v[4].value)

    def diag(self):
        """what the last train decided (nle_filter_diag): formulation taken, ranks kept by the three 1e-10 cuts"""
        v = np.zeros(8, dtype=np.int32)
        _check(lib().nle_filter_diag(self._f, _np_ptr(v)))
        keys = ("formulation", "p", "r_Ka", "r_Wa", "r_Q", "K", "chol_Ka", "chol_Wa")
        return {k: int(x) for k, x in zip(keys, v)}

    def chroma(self):
        """the chroma bandwidth hc the filter was trained with, 0.0 without (nle_filter_chroma)"""
        hc = C.c_double()
        _check(lib().nle_filter_chroma(self._f, C.byref(hc)))
        return hc.value

    @property
    def eigvals(self):
        K = self.info()["K"]
        out = np.zeros(K, dtype=np.float64)
        _check(lib().nle_filter_eigvals(self._f, _np_ptr(out)))
        return out

    def sample_pixels(self):
        """the sample set the filter was trained on (nle_filter_sample_pixels): row-major pixel indices, ascending"""
        p = C.c_int()
        _check(lib().nle_filter_sample_pixels(self._f, None, C.byref(p)))
        out = np.zeros(p.value, dtype=np.int64)
        _check(lib().nle_filter_sample_pixels(self._f, _np_ptr(out), C.byref(p)))
        return out

    def eigvecs(self):
        """m_eigvecs as a CUDA tensor view (n_local x ld(K)), pixel order."""
        torch = _torch()
        ptr, ldv = C.c_void_p(), C.c_int()
        _check(lib().nle_filter_eigvecs(self._f, C.byref(ptr), C.byref(ldv)))
        n = self.info()["n_local"]
        out = torch.empty((n, ldv.value), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        _check(lib().nle_filter_copy_eigvecs(self._f, C.c_void_p(out.data_ptr())), self.ctx._h)
        return out

    def eigvec_range(self, ncols):
        """(min, max) of the first `ncols` eigenvector columns over this rank's pixels (the banner of
        src/filter.cpp:506); does not materialise an implicit V"""
        mn = np.zeros(ncols, dtype=np.float64)
        mx = np.zeros(ncols, dtype=np.float64)
        _check(lib().nle_filter_eigvec_range(self._f, int(ncols), _np_ptr(mn), _np_ptr(mx)), self.ctx._h)
        return mn, mx

    def timings(self):
        ms = np.zeros(6)
        _check(lib().nle_filter_timings(self._f, _np_ptr(ms)))
        return dict(zip(("setup", "sinkhorn", "gram", "project", "host", "total"), ms.tolist()))

    def apply(self, x, f_s, out=None):
        """`NLEFilter::apply` (src/filter.cpp:445-458): y = V diag(fS) V^T x (local slab)."""
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = self._full_shape(x, self.shape)
        fs = np.ascontiguousarray(f_s, dtype=np.float64)
        if fs.ndim != 1 or fs.size != self.info()["K"]:   # nle_apply reads K doubles
            raise NLEError(NLE_ERR_INVALID, f"f_s must hold K' = {self.info()['K']} values, got {fs.shape}")
        n = self.info()["n_local"]
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=x.device)
        _check(lib().nle_apply(self._f, C.c_void_p(x.data_ptr()), H, W, _np_ptr(fs), C.c_void_p(out.data_ptr())),
               self.ctx._h)
        return out

    def _planes(self, planes, one_ok):
        """planes as a P x H x W float32 device tensor, each plane contiguous, any stride >= H W between them (one_ok: one
        H x W plane is taken as P = 1) -> (tensor, P, H, W)"""
        torch = _torch()
        t = torch.as_tensor(planes, dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        if one_ok and t.ndim == 2:
            t = t[None]
        if t.ndim != 3:
            raise NLEError(NLE_ERR_INVALID, "planes must be P x H x W")
        P, H, W = t.shape
        if t.stride(2) != 1 or t.stride(1) != W or (P > 1 and t.stride(0) < H * W):
            t = t.contiguous()
        self.ctx._sync_in()
        return t, P, H, W

    def apply_planes(self, planes, responses, out_kind=0, out=None):
        """nle_apply_planes: the filter applied to P planes in one call, each with its own responses; every output is bit
        for bit what `apply` / `apply_layers` / `apply_rounded8` give plane by plane.

        planes: P x H x W float32 (a device tensor may have any stride between its planes; each plane is contiguous).
        responses: per plane a (K',) vector or an (L_m, K') array (1 <= L_m <= 64), R = sum L_m <= 128; None: one response
        of ones for every plane.  out_kind: REGION_OUT_F32 or REGION_OUT_ROUNDED8.  Returns (R, n_local) float32, the
        outputs of plane 0 first; `out` may be such a tensor with any stride between its rows."""
        torch = _torch()
        t, P, H, W = self._planes(planes, one_ok=False)
        K = self.info()["K"]
        if responses is None:
            responses = [np.ones(K)] * P
        if len(responses) != P:
            raise NLEError(NLE_ERR_INVALID, f"one set of responses per plane expected: {P} planes, {len(responses)} sets")
        rows = [np.atleast_2d(np.asarray(r, dtype=np.float64)) for r in responses]
        for r in rows:
            if r.ndim != 2 or r.shape[1] != K:   # nle_apply_planes reads K' doubles per response
                raise NLEError(NLE_ERR_INVALID, f"every response must hold K' = {K} values, got {r.shape}")
        nresp = np.ascontiguousarray([r.shape[0] for r in rows], dtype=np.int32)
        resp = np.ascontiguousarray(np.concatenate(rows, axis=0))
        R, n = int(nresp.sum()), self.info()["n_local"]
        if out is None:
            out = torch.empty((R, n), dtype=torch.float32, device=t.device)
        elif tuple(out.shape) != (R, n) or out.dtype != torch.float32 or out.stride(1) != 1:
            raise NLEError(NLE_ERR_INVALID, f"out must be a float32 tensor of shape {(R, n)} with contiguous rows")
        _check(lib().nle_apply_planes(self._f, C.c_void_p(t.data_ptr()), P, t.stride(0) if P > 1 else H * W, H, W,
                                      _np_ptr(nresp), _np_ptr(resp), int(out_kind), C.c_void_p(out.data_ptr()),
                                      out.stride(0) if R > 1 else n), self.ctx._h)
        return out

    def coefficients(self, planes):
        """nle_filter_coefficients: t = V^T x of P planes (P x H x W float32, or one H x W plane) as a (P, K') float64 array,
        row m bit for bit the vector `apply` forms for plane m"""
        t, P, H, W = self._planes(planes, one_ok=True)
        out = np.zeros((max(P, 1), self.info()["K"]))
        _check(lib().nle_filter_coefficients(self._f, C.c_void_p(t.data_ptr()), P, t.stride(0) if P > 1 else H * W, H, W,
                                             _np_ptr(out)), self.ctx._h)
        return out

    def _strokes(self, strokes):
        torch = _torch()
        t = torch.as_tensor(strokes, dtype=torch.float32, device=f"cuda:{self.ctx.device}").contiguous()
        if t.ndim != 3:
            raise NLEError(NLE_ERR_INVALID, "strokes must be M x H x W")
        self.ctx._sync_in()
        return t

    @staticmethod
    def _scale(scale, M):
        if scale is None:
            return None, None
        c = np.ascontiguousarray(scale, dtype=np.float64)
        if c.shape != (M,):
            raise NLEError(NLE_ERR_INVALID, f"scale must hold M = {M} values, got {c.shape}")
        return c, _np_ptr(c)

    def region_spread(self, strokes, scale=None, spread=4.0, out=None):
        """nle_region_spread: q_m = apply(s_m, c_m lambda^spread) for the M stroke planes (M x H x W); scale: the M values
        c_m or None (1).  Returns (M, n_local) float32."""
        torch = _torch()
        s = self._strokes(strokes)
        M, H, W = s.shape
        c, cp = self._scale(scale, M)
        if out is None:
            out = torch.empty((M, self.info()["n_local"]), dtype=torch.float32, device=s.device)
        _check(lib().nle_region_spread(self._f, C.c_void_p(s.data_ptr()), M, H, W, cp, float(spread),
                                       C.c_void_p(out.data_ptr())), self.ctx._h)
        return out

    def apply_regions(self, x, n_layers, strokes, weights, scale=None, spread=4.0, floor=0.05, out_kind=0, out=None):
        """nle_apply_regions: the layers of x, the spreads of the stroke planes and the combine in one call.  weights:
        (M + 1, n_layers) float64, row 0 the background.  Returns n_local float32 values, or bytes for REGION_OUT_U8."""
        x = self.ctx._lum(x)
        H, W = x.shape
        s = self._strokes(strokes)
        M = s.shape[0]
        c, cp = self._scale(scale, M)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (M + 1, int(n_layers)):
            raise NLEError(NLE_ERR_INVALID, f"weights must be {(M + 1, int(n_layers))}, got {w.shape}")
        out = _combine_out(out, self.info()["n_local"], out_kind, x.device)
        _check(lib().nle_apply_regions(self._f, C.c_void_p(x.data_ptr()), H, W, int(n_layers), C.c_void_p(s.data_ptr()), M,
                                       cp, float(spread), float(floor), _np_ptr(w), int(out_kind),
                                       C.c_void_p(out.data_ptr())), self.ctx._h)
        return out

    def apply_local(self, x, n_layers, strokes, weights, detail=None, curves=None, scale=None, spread=4.0, floor=0.05,
                    out_kind=0, out=None, want_spreads=False):
        """nle_apply_local: the layers of x, the spreads of the stroke planes and the local combine in one call.  weights,
        detail and curves as for Context.local_combine.  want_spreads: (out, q) with q the (M, n_local) spreads, the membership
        planes Context.local_chroma takes.  Returns n_local float32 values, or bytes for REGION_OUT_U8."""
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = x.shape
        s = self._strokes(strokes)
        M = s.shape[0]
        c, cp = self._scale(scale, M)
        w, d, on, cv = _local_rows("apply_local", M, int(n_layers), weights, detail, curves)
        n = self.info()["n_local"]
        out = _combine_out(out, n, out_kind, x.device)
        q = torch.empty((M, n), dtype=torch.float32, device=x.device) if want_spreads else None
        _check(lib().nle_apply_local(self._f, C.c_void_p(x.data_ptr()), H, W, int(n_layers), C.c_void_p(s.data_ptr()), M, cp,
                                     float(spread), float(floor), _np_ptr(w), _np_ptr(d), _np_ptr(on) if on is not None else None,
                                     _np_ptr(cv) if cv is not None else None, int(out_kind), C.c_void_p(out.data_ptr()),
                                     C.c_void_p(q.data_ptr()) if q is not None else None), self.ctx._h)
        return (out, q) if want_spreads else out

    def apply_local_auto(self, x, n_layers, strokes, weights, tone, detail=None, scale=None, spread=4.0, floor=0.05,
                         out_kind=0, out=None, want_spreads=False, want_curves=False):
        """nle_apply_local_auto: apply_local with every row's base curve made from the row's own membership-weighted
        histogram.  tone (M + 1, 4) = (shadows, highlights, clip_percent, equalise) per row, in tone_curve's ranges; a row of
        (0, 0, -1, 0) has no curve.  Returns the output, then -- want_spreads -- the (M, n_local) spreads and -- want_curves --
        the (M + 1, TONE_KNOTS + 2) curves (zeros for a row without one)."""
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = x.shape
        s = self._strokes(strokes)
        M = s.shape[0]
        c, cp = self._scale(scale, M)
        w, d, _, _ = _local_rows("apply_local_auto", M, int(n_layers), weights, detail, None)
        tn = np.ascontiguousarray(tone, dtype=np.float64)
        if tn.shape != (M + 1, 4):
            raise NLEError(NLE_ERR_INVALID, f"apply_local_auto: tone must be {(M + 1, 4)}, got {tn.shape}")
        n = self.info()["n_local"]
        out = _combine_out(out, n, out_kind, x.device)
        q = torch.empty((M, n), dtype=torch.float32, device=x.device) if want_spreads else None
        cv = np.zeros((M + 1, TONE_KNOTS + 2)) if want_curves else None
        _check(lib().nle_apply_local_auto(self._f, C.c_void_p(x.data_ptr()), H, W, int(n_layers), C.c_void_p(s.data_ptr()), M, cp,
                                          float(spread), float(floor), _np_ptr(w), _np_ptr(d), _np_ptr(tn), int(out_kind),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(q.data_ptr()) if q is not None else None,
                                          _np_ptr(cv) if cv is not None else None), self.ctx._h)
        res = (out,) + ((q,) if want_spreads else ()) + ((cv,) if want_curves else ())
        return res if len(res) > 1 else out

    def segment(self, count, spread=4.0, max_iter=40, labels=None, want_spreads=False):
        """nle_filter_segment: kernel k-means of the pixels on the trained affinity, `count` clusters.  labels: the start, n
        uint8 values (a device tensor is REWRITTEN in place); None: the equal-population start (Context.segment_init) on the
        plane train_filter was given.  Returns a dict: labels (n uint8 on the device), counts, objective (one value per
        iteration made), iterations, converged, and -- want_spreads -- spreads, the (count, n) float32 spreads of the
        returned labels (the membership planes Context.region_combine takes)."""
        torch = _torch()
        H, W = self.shape
        if labels is None:
            if self._train_plane is None:
                raise NLEError(NLE_ERR_INVALID, "segment: no start labels given and the training plane is not on the device")
            labels, _ = self.ctx.segment_init(self._train_plane, count)
        Cn, n = int(count), H * W
        labels = self.ctx._labels(labels, "segment", n)
        self.ctx._sync_in()
        q = torch.empty((max(Cn, 1), n), dtype=torch.float32, device=labels.device) if want_spreads else None
        counts, obj = np.zeros(max(Cn, 1), dtype=np.int64), np.full(max(int(max_iter), 1), np.nan)
        iters, conv = C.c_int(0), C.c_int(0)
        _check(lib().nle_filter_segment(self._f, H, W, Cn, float(spread), int(max_iter), C.c_void_p(labels.data_ptr()),
                                        C.c_void_p(q.data_ptr()) if q is not None else None, n, _np_ptr(counts), _np_ptr(obj),
                                        C.byref(iters), C.byref(conv)), self.ctx._h)
        out = dict(labels=labels, counts=counts[:Cn], objective=obj[:iters.value], iterations=iters.value,
                   converged=bool(conv.value))
        if want_spreads:
            out["spreads"] = q
        return out

    def apply_detail(self, x, weights, residual_weight=0.0, gain=1.0, sigma=0.0, out_kind=0, out=None):
        """nle_apply_detail: the len(weights) layers of x and the detail combine in one call -- the out-of-span residual
        x - sum of the layers as one more layer under residual_weight, and the gain curve (gain, sigma) on the residual and
        on every layer but the last.  Returns n_local float32 values, or bytes for REGION_OUT_U8."""
        x = self.ctx._lum(x)
        H, W = x.shape
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 1:
            raise NLEError(NLE_ERR_INVALID, f"weights must be a vector, got {w.shape}")
        out = _combine_out(out, self.info()["n_local"], out_kind, x.device)
        _check(lib().nle_apply_detail(self._f, C.c_void_p(x.data_ptr()), H, W, int(w.shape[0]), _np_ptr(w),
                                      float(residual_weight), float(gain), float(sigma), int(out_kind),
                                      C.c_void_p(out.data_ptr())), self.ctx._h)
        return out

    def apply_tone(self, x, weights, residual_weight=0.0, gain=1.0, sigma=0.0, shadows=0.0, highlights=0.0, clip_percent=-1.0,
                   equalise=0.0, out_kind=0, out=None, want_curve=False):
        """nle_apply_tone: apply_detail with the base layer passed through the tone curve of (shadows, highlights,
        clip_percent, equalise) -- the layers, the histogram of the weighted base layer where the curve needs it, the curve
        and the combine in one call.  All four at their defaults: apply_detail, bit for bit.  want_curve: (out, curve)."""
        x = self.ctx._lum(x)
        H, W = x.shape
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 1:
            raise NLEError(NLE_ERR_INVALID, f"weights must be a vector, got {w.shape}")
        out = _combine_out(out, self.info()["n_local"], out_kind, x.device)
        curve = np.zeros(TONE_KNOTS + 2)
        _check(lib().nle_apply_tone(self._f, C.c_void_p(x.data_ptr()), H, W, int(w.shape[0]), _np_ptr(w),
                                    float(residual_weight), float(gain), float(sigma), float(shadows), float(highlights),
                                    float(clip_percent), float(equalise), int(out_kind), C.c_void_p(out.data_ptr()),
                                    _np_ptr(curve) if want_curve else None), self.ctx._h)
        return (out, curve) if want_curve else out

    def apply_layers(self, x, n_layers, out=None):
        torch = _torch()
        x = self.ctx._lum(x)
        H, W = self._full_shape(x, self.shape)
        n = self.info()["n_local"]
        if out is None:
            out = torch.empty((n_layers, n), dtype=torch.float32, device=x.device)
        _check(lib().nle_apply_layers(self._f, C.c_void_p(x.data_ptr()), H, W, int(n_layers),
                                      C.c_void_p(out.data_ptr())), self.ctx._h)
        return out
