"""The Dense kernels (csrc/dense.hip: forward with bias / ReLU and its K split, data gradient, weight gradient) through the C ABI,
ELEMENT BY ELEMENT against tests/dense_ref.py, on every path the host code can take: both tile geometries (64 x 64, and 128 x 128
from 256 tiles of 128 x 128 on), the vector and the scalar loaders (odd sizes AND a base pointer one float off a 16-byte boundary),
K tails, ragged tiles, the forward's K split with 8, 9, 13, 14, 16 and 58 slabs, and the unsplit fallback taken without a workspace.

tests/test_backbone_gpu.py::test_dense_gap_add_l2 judges four shapes by max |err| / max |ref| of the whole tensor;
tests/test_dense_ref_cpu.py shows what that lets through (a bias read from the neighbouring column, an error confined to a quiet
column, operands silently cut to 16 bits).  Here every case runs two operand families (dense_ref.operands):

  ints   integers in [-3, 3]: every sum is exact in fp32 in any order -> the kernel's result EQUALS the float64 one, bit for bit
         (a wrong row, column, bias column, dropped k or slab changes an integer);
  reals  randn with quiet columns / rows, a zero column and row -> dense_ref.check_elementwise for every element:
         |got - f64| <= (K + extra) 2^-24 mag / (1 - (K + extra) 2^-24), the a-priori bound of fp32 accumulation in any order
         (extra = slab adds + the bias add); |got - f64| / mag <= max(2 E32, 5e-7), E32 the k-ordered float32 chain's own largest
         error / mag on the same operands; exactly 0 where mag = 0.

Every output is written into a NaN-filled buffer between two NaN guard bands of 256 floats, which must stay NaN; operands sit
between NaN pads, the K-split workspace starts as NaN.

Measured on an MI355X: the largest |got - f64| / mag of the `reals` family as a multiple of E32 (the assertion allows 2, or 5e-7
absolute), by pass and path; `ints` is bit-exact on every path, and the 128 x 128 and the 64 x 64 geometry give the same bits on
their common elements for `reals` too:

  path                                  fwd   dgrad   wgrad
  G64 scalar                           2.42*   1.18    1.08
  G64 vec                              1.06    1.19    1.03
  G64 scalar (pointer + 4 bytes)       0.83    1.00    1.03
  G64 vec, 225 tiles of 128            1.14       -    1.02
  G128 scalar                          1.14       -    1.02
  G128 vec                             1.11    1.05    0.95
  split-K scalar                       0.23       -       -
  split-K vec                          0.38       -       -
  G64 scalar, long K (no workspace)    1.00       -       -
  G64 vec, long K (no workspace)       1.20       -       -

  * (3, 33, 5) with bias: 8.2e-8 against E32 = 3.4e-8, i.e. under the 5e-7 floor and 25 times under the a-priori bound.  Fifteen
    elements, two summation orders (the engine's k schedule inside a K tile is not k order): the larger of fifteen rounding errors
    of one order against the other, not a defect — the bias column, the tails and every index are pinned by `ints` at the same shape.
    Every other case stays at or below 1.20; the K split's slabs shorten the chains (0.23 - 0.38).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd import layers as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                                               # floats of NaN on each side of every output
PAD = 4                                                   # floats of NaN on each side of every operand (keeps 16-byte alignment)
NAN = float("nan")
RATIOS = {}                                               # (pass, path) -> largest ratio to E32 seen


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    yield torch.device("cuda", 0)
    if RATIOS:
        print("\nDENSE RATIO TABLE  largest |got - f64| / mag as a multiple of E32 (reals)")
        for (kind, path), r in sorted(RATIOS.items()):
            print("DENSE RATIO  %-6s %-34s %.2f" % (kind, path, r))


def no_split_override():
    if os.environ.get("EMBNET_DENSE_SPLIT_MIN_KT"):
        pytest.skip("EMBNET_DENSE_SPLIT_MIN_KT is set: the K-split plan this case pins is not the default one")


def cdiv(a, b):
    return -(-a // b)


def uses_g128(rows, cols):
    """LAUNCH_DENSE: the 128 x 128 geometry from 256 tiles of 128 x 128 on (rows x cols: the OUTPUT of the pass)."""
    return cdiv(rows, 128) * cdiv(cols, 128) >= 256


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
def place(a, dev, shift=0):
    """a on the device between NaN pads; shift: floats by which its first element is off a 16-byte boundary."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * PAD + shift,), NAN, device=dev)
    view = buf[PAD + shift:PAD + shift + a.size]
    view.copy_(torch.tensor(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 * shift
    return view


def guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), NAN, device=dev)
    out = buf[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    return buf, out


def collect(buf, n, shape, what):
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + n:]).all(), "%s wrote outside its output" % what
    return host[GUARD:GUARD + n].reshape(shape).copy()


def traced(call):
    """Run call() with the library's launch trace on -> the kernel names it launched."""
    _lib.trace_reset(); _lib.trace_enable(True)
    try:
        call()
        torch.cuda.synchronize()
        return [r[0] for r in _lib.trace_records()]
    finally:
        _lib.trace_enable(False)


# ---- the three entry points ------------------------------------------------------------------------------------------------------------
def run_fwd(dev, x, w, bias, relu, workspace=True, shift_x=0, shift_w=0):
    """-> (y [m, out], split: whether the finish kernel ran).  workspace False: none is passed (the unsplit fallback)."""
    lib = _lib.lib()
    (m, i), o = x.shape, w.shape[1]
    xd, wd, bd = place(x, dev, shift_x), place(w, dev, shift_w), place(bias, dev)
    buf, y = guarded(m * o, dev)
    nws = lib.embnet_dense_fwd_workspace_bytes(m, i, o) if workspace else 0
    ws = torch.full((nws // 4,), NAN, device=dev) if nws else None
    names = traced(lambda: _lib.check(lib.embnet_dense_fwd_f32(
        xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, y.data_ptr(), m, i, o, int(relu),
        ws.data_ptr() if nws else None, nws, _lib.stream())))
    assert any("dense_fwd_kernel" in s for s in names), names
    return collect(buf, m * o, (m, o), "dense_fwd"), any("dense_splitk_finish_kernel" in s for s in names)


def run_dgrad(dev, dy, w, shift_dy=0, shift_w=0):
    lib = _lib.lib()
    (m, o), i = dy.shape, w.shape[0]
    dyd, wd = place(dy, dev, shift_dy), place(w, dev, shift_w)
    buf, dx = guarded(m * i, dev)
    names = traced(lambda: _lib.check(lib.embnet_dense_dgrad_f32(dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), m, i, o, _lib.stream())))
    assert any("dense_dgrad_kernel" in s for s in names), names
    return collect(buf, m * i, (m, i), "dense_dgrad")


def run_wgrad(dev, x, dy, shift_x=0, shift_dy=0):
    lib = _lib.lib()
    (m, i), o = x.shape, dy.shape[1]
    xd, dyd = place(x, dev, shift_x), place(dy, dev, shift_dy)
    buf, dw = guarded(i * o, dev)
    names = traced(lambda: _lib.check(lib.embnet_dense_wgrad_f32(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), m, i, o, _lib.stream())))
    assert any("dense_wgrad_kernel" in s for s in names), names
    return collect(buf, i * o, (i, o), "dense_wgrad")


# ---- references, computed once per (family, shape) and left unchanged ----------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def operands(family, shape):
    out = DR.operands(family, DR.seed_of(shape), *shape)
    for t in out[:4]:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=6)
def chain(kind, family, shape):
    x, w, bias, dy, _ = operands(family, shape)
    a, b = DR.pass_problem(kind, x, w, bias, dy)[:2]
    acc = DR.chain32(a, b)
    acc.setflags(write=False)
    return acc


FWD_MODES = [(True, True), (True, False), (False, False)]                    # (bias, ReLU): bias + ReLU, bias only, neither


def judge(kind, path, shape, family, got, with_bias=False, relu=False, slab_adds=0, crop=None):
    """got against the float64 result of pass `kind` on operands(family, shape).  crop (rows, cols): got covers only that top-left
    part of the output (the operands were cut accordingly; the reduction is whole)."""
    x, w, bias, dy, _ = operands(family, shape)
    _, _, f64, mag, k = DR.pass_problem(kind, x, w, bias, dy, with_bias, relu)
    ref32 = DR.epilogue32(chain(kind, family, shape), bias if with_bias else None, relu) if family == "reals" else None
    if crop is not None:
        f64, mag = f64[:crop[0], :crop[1]], mag[:crop[0], :crop[1]]
        ref32 = ref32[:crop[0], :crop[1]] if ref32 is not None else None
    what = "%s %s %s %s%s%s" % (kind, "x".join(map(str, shape)), path, family, " +bias" if with_bias else "", " +relu" if relu else "")
    assert got.shape == f64.shape, (what, got.shape, f64.shape)
    if family == "ints":
        bad = got.astype(np.float64) != f64                  # (NaN != anything: an element never written counts)
        assert not bad.any(), "%s: %d of %d elements differ from the exact result, first at %s: %r != %r" % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], f64[tuple(np.argwhere(bad)[0])])
        return
    e32 = DR.e32_of(ref32, f64, mag)
    ratio = DR.check_elementwise(got, f64, mag, k, slab_adds + int(with_bias), e32, what)
    print("DENSE ELEMENTWISE %s: |got - f64| / mag = %.2f x E32 (%.2e)" % (what, ratio, e32))
    if np.isfinite(ratio):
        RATIOS[(kind, path)] = max(RATIOS.get((kind, path), 0.0), ratio)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_pass(dev, kind, family, shape, path, **kw):
    """One pass on operands(family, shape), every forward mode, judged.  -> the results (forward: one per mode)."""
    x, w, bias, dy, _ = operands(family, shape)
    if kind == "fwd":
        outs = []
        for with_bias, relu in FWD_MODES:
            y, split = run_fwd(dev, x, w, bias if with_bias else None, relu, **kw)
            assert not split, "%s: not expected to take the K split" % (shape,)
            judge("fwd", path, shape, family, y, with_bias, relu)
            outs.append(y)
        return outs
    got = run_dgrad(dev, dy, w, **kw) if kind == "dgrad" else run_wgrad(dev, x, dy, **kw)
    judge(kind, path, shape, family, got)
    return got


# ---- the 64 x 64 geometry: smallest shapes, tails, both loaders ---------------------------------------------------------------------------
# (m, in, out); vec = the float4 loaders: forward and weight gradient need in % 4 == 0 and out % 4 == 0, the data gradient out % 4 == 0.
# All: one to four 64 x 64 tiles, no K split (fewer than 64 K tiles).
#   (1, 1, 1)     scalar; one element, one product
#   (3, 33, 5)    scalar; two K tiles, the second holds ONE element (forward); data gradient K = 5, weight gradient K = 3
#   (67, 31, 66)  scalar; K < BK (forward), 2 x 2 ragged tiles (forward); data gradient 2 x 1 tiles, K = 66 = 2 tiles + 2
#   (64, 32, 64)  vec; exactly one tile and one K tile (forward); nothing ragged anywhere
#   (65, 36, 68)  vec; 2 x 2 ragged tiles, K = 36: a tail of 4 (forward); data gradient K = 68: tail of 4; weight gradient K = 65: tail of 1
#   (5, 70, 33)   scalar; the shape tests/test_backbone_gpu.py has
#   (7, 33, 36)   data gradient vec (out % 4 == 0) with an odd number of rows in w; forward and weight gradient scalar
G64_SHAPES = DR.G64_SHAPES + [(7, 33, 36)]


def loaders(kind, shape):
    m, i, o = shape
    vec = (o % 4 == 0) if kind == "dgrad" else (i % 4 == 0 and o % 4 == 0)
    return "vec" if vec else "scalar"


def out_dims(kind, shape):
    m, i, o = shape
    return {"fwd": (m, o), "dgrad": (m, i), "wgrad": (i, o)}[kind]


@pytest.mark.parametrize("family", DR.FAMILIES)
@pytest.mark.parametrize("shape", G64_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_g64_tails_and_loaders(dev, shape, family):
    assert _lib.lib().embnet_dense_fwd_workspace_bytes(*shape) == 0
    for kind in ("fwd", "dgrad", "wgrad"):
        assert not uses_g128(*out_dims(kind, shape))
        run_pass(dev, kind, family, shape, "G64 " + loaders(kind, shape))


# ---- a 4-divisible shape on a pointer one float off: the scalar loaders with ld % 4 == 0 ---------------------------------------------------
@pytest.mark.parametrize("family", DR.FAMILIES)
def test_misaligned_operands_take_the_scalar_loaders(dev, family):
    shape = DR.MISALIGNED_SHAPE                              # (8, 64, 64): vec when aligned; one tile, two K tiles
    path = "G64 scalar (pointer + 4 bytes)"
    aligned = {kind: run_pass(dev, kind, family, shape, "G64 vec") for kind in ("fwd", "dgrad", "wgrad")}
    for kind, shifts in (("fwd", ({"shift_x": 1}, {"shift_w": 1})), ("dgrad", ({"shift_dy": 1}, {"shift_w": 1})),
                         ("wgrad", ({"shift_x": 1}, {"shift_dy": 1}))):
        for kw in shifts:
            got = run_pass(dev, kind, family, shape, path, **kw)
            if family == "ints":
                for g, a in zip(got if kind == "fwd" else [got], aligned[kind] if kind == "fwd" else [aligned[kind]]):
                    assert same_bits(g, a), (kind, kw)


# ---- the forward's K split ------------------------------------------------------------------------------------------------------------------
# dense_fwd_plan: tiles = cdiv(m, 64) cdiv(out, 64) < 64 and kt = cdiv(in, 32) >= 64 -> want = min(512 / tiles, kt / 4) slabs of
# cdiv(kt, want) K tiles.  The finish kernel adds slabs 1.. eight at a time, then one at a time.
#   (8, 2048, 128)    vec; 2 tiles, 64 K tiles, 16 slabs of 4: one unrolled round + 7
#   (5, 2050, 33)     scalar; 1 tile, 65 K tiles (tail of 2), 13 slabs of 5: one unrolled round + 4
#   (6, 2116, 36)     vec; 1 tile, 67 K tiles (tail of 4), 14 slabs of 5, the last of 2 K tiles: one unrolled round + 5
#   (960, 2048, 256)  vec; 60 tiles, 64 K tiles, 8 slabs of 8: no unrolled round, 7 in the remainder loop
#   (200, 2052, 800)  vec; 4 x 13 = 52 ragged tiles, 65 K tiles (tail of 4), want 9 -> 9 slabs of 8, the last of ONE K tile holding
#                     4 elements: exactly one unrolled round, no remainder
@pytest.mark.parametrize("family", DR.FAMILIES)
@pytest.mark.parametrize("shape,slabs", DR.SPLITK_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_split_k_forward_and_its_unsplit_fallback(dev, shape, slabs, family):
    no_split_override()
    m, i, o = shape
    assert _lib.lib().embnet_dense_fwd_workspace_bytes(m, i, o) // (4 * m * o) == slabs
    assert _lib.lib().embnet_dense_fwd_workspace_bytes(m, i, o) == 4 * m * o * slabs
    x, w, bias, dy, _ = operands(family, shape)
    vec = loaders("fwd", shape)
    for with_bias, relu in FWD_MODES:
        y, split = run_fwd(dev, x, w, bias if with_bias else None, relu)
        assert split, "the finish kernel did not run"
        judge("fwd", "split-K %s" % vec, shape, family, y, with_bias, relu, slab_adds=slabs - 1)
        y0, split = run_fwd(dev, x, w, bias if with_bias else None, relu, workspace=False)
        assert not split, "no workspace was passed, yet the finish kernel ran"
        judge("fwd", "G64 %s, long K (no workspace)" % vec, shape, family, y0, with_bias, relu)
        if family == "ints":
            assert same_bits(y, y0)


# ---- the 128 x 128 geometry ----------------------------------------------------------------------------------------------------------------
# LAUNCH_DENSE takes it at cdiv(rows, 128) cdiv(cols, 128) >= 256 of the pass's output: 16 x 16 tiles here, ragged by 5 / 3 (scalar,
# odd sizes) or 8 / 4 (vec); K = 36 (two K tiles, tail of 4).  1920 x 1920 is 15 x 15 = 225 tiles of 128: the 64 x 64 geometry, on
# the top-left part of the same operands — the two geometries must give the same elements.
@pytest.mark.parametrize("family", DR.FAMILIES)
@pytest.mark.parametrize("kind,shape", DR.G128_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_g128_geometry_and_its_g64_neighbour(dev, kind, shape, family):
    assert uses_g128(*out_dims(kind, shape)) and _lib.lib().embnet_dense_fwd_workspace_bytes(*shape) == 0
    big = run_pass(dev, kind, family, shape, "G128 " + loaders(kind, shape))
    if kind == "dgrad":
        return
    m, i, o = shape
    x, w, bias, dy, _ = operands(family, shape)
    n = DR.BELOW_G128[0]                                     # 1920
    assert not uses_g128(n, n)
    path = "G64 vec, 225 tiles of 128"
    if kind == "fwd":
        for (with_bias, relu), yb in zip(FWD_MODES, big):
            y, split = run_fwd(dev, x[:n], w[:, :n], bias[:n] if with_bias else None, relu)
            assert not split
            judge("fwd", path, shape, family, y, with_bias, relu, crop=(n, n))
            print("DENSE G128 == G64 on the common part, bit for bit (%s fwd): %s" % (family, same_bits(y, yb[:n, :n])))
            assert family != "ints" or same_bits(y, yb[:n, :n])
    else:
        dw = run_wgrad(dev, x[:, :n], dy[:, :n])
        judge("wgrad", path, shape, family, dw, crop=(n, n))
        print("DENSE G128 == G64 on the common part, bit for bit (%s wgrad): %s" % (family, same_bits(dw, big[:n, :n])))
        assert family != "ints" or same_bits(dw, big[:n, :n])


# ---- the workload's own head, Flatten -> Dense(512) of simple2, at its smallest batch ------------------------------------------------------------
# forward: 8 tiles, 400 K tiles -> 58 slabs of 7 (the last of 1): seven unrolled rounds + 1; data gradient: 1 x 200 tiles of 64 x 64,
# K = 512; weight gradient: 100 x 4 = 400 tiles of 128 x 128 -> G128, K = 4 (one K tile holding four elements)
@pytest.mark.parametrize("family", DR.FAMILIES)
def test_the_simple2_head_at_batch_4(dev, family):
    no_split_override()
    shape = DR.HEAD_SHAPE
    m, i, o = shape
    assert _lib.lib().embnet_dense_fwd_workspace_bytes(m, i, o) // (4 * m * o) == DR.HEAD_SLABS
    assert not uses_g128(m, i) and uses_g128(i, o)
    x, w, bias, dy, _ = operands(family, shape)
    for with_bias, relu in FWD_MODES:
        y, split = run_fwd(dev, x, w, bias if with_bias else None, relu)
        assert split
        judge("fwd", "split-K vec", shape, family, y, with_bias, relu, slab_adds=DR.HEAD_SLABS - 1)
    run_pass(dev, "dgrad", family, shape, "G64 vec")
    run_pass(dev, "wgrad", family, shape, "G128 vec")


# ---- through the layer: non-zero bias, ReLU, the gradients of an exact-zero pre-activation -----------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 36, 68), (6, 2116, 36)], ids=lambda s: "x".join(map(str, s)))
def test_dense_layer_with_bias_and_relu_is_exact_on_integers(dev, shape):
    m, i, o = shape
    x, w, bias, dy, _ = DR.operands("ints", DR.seed_of(shape) + 7, m, i, o)
    z = DR.fwd64(x, w)
    forced = [(c % m, c) for c in range(4)]                  # four pre-activations made EXACTLY zero by their column's bias,
    for r, c in forced:                                      # under a non-zero incoming gradient
        bias[c] = -z[r, c]
        dy[r, c] = 3.0
    assert np.abs(z).max() + np.abs(bias).max() < 2 ** 24 and 2 * np.count_nonzero(bias) > o
    z = z + bias.astype(np.float64)[None, :]
    assert all(z[r, c] == 0 for r, c in forced)
    dz = np.where(z > 0, dy.astype(np.float64), 0.0)         # ReLU passes no gradient at 0
    want = {"y": np.maximum(z, 0), "dx": dz @ w.astype(np.float64).T, "dw": x.astype(np.float64).T @ dz, "db": dz.sum(0)}
    assert max(np.abs(v).max() for v in want.values()) < 2 ** 24
    d = L.Dense(i, o, activation="relu", gen=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        d.kernel.copy_(torch.from_numpy(w).to(dev))
        d.bias.copy_(torch.from_numpy(bias).to(dev))
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    y = d(xt)
    y.backward(torch.from_numpy(dy).to(dev))
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xt.grad, "dw": d.kernel.grad, "db": d.bias.grad}
    for name, ref in want.items():
        g = got[name].cpu().numpy().astype(np.float64)
        assert g.shape == ref.shape and np.array_equal(g, ref), (name, shape, int((g != ref).sum()))
