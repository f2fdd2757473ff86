"""tests/dense_ref.py proves itself, without a GPU: the comparator accepts the float32 chain it is built on, at every shape of
tests/test_dense_elementwise_gpu.py and for both operand families, and REJECTS outputs made wrong on purpose — the errors a Dense
kernel can make at a tail tile, a K tail, the bias pre-load or the K-split finish.  For each wrong output the metric the suite had
before (tests/test_backbone_gpu.py::test_dense_gap_add_l2: max |err| / max |ref| over the tensor against 2e-5 sqrt(in / 2048)) is
computed too, and the test prints which of them it would have let through.  On the `reals` family, over the forward shapes below
(batch capped so that a case stays near a second):

  wrong output           rejected per element    the old metric
  bias_rolled            every shape             lets it through at every shape (4e-7 .. 8.6e-6 against 2e-5)
  quiet_column_last_k    every shape             lets it through at 12 of 15 shapes, at every in >= 2048 (asserted there: one product
                                                 of K in a column 2^-12 down is about 3 x 2^-12 / sqrt(K) of the loudest result)
  bf16x2                 every shape             lets it through at 11 of 16 shapes (1.2e-5 .. 2.4e-5: it sits AT the tolerance)
  last_k_dropped         every shape             catches it (3.5e-3 .. 1)
  last_row_repeats       every shape             catches it
  slab_left_out          every shape             catches it

`ints` outputs are judged by equality, so every wrong output that differs at all is rejected there (bf16x2 cannot differ: integers
in [-3, 3] are bf16 numbers).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as DR  # noqa: E402

SMALL = DR.G64_SHAPES + [DR.MISALIGNED_SHAPE] + [s for s, _ in DR.SPLITK_SHAPES] + [DR.BELOW_G128, DR.HEAD_SHAPE]
PASS_CASES = [(kind, s) for s in SMALL for kind in ("fwd", "dgrad", "wgrad")] + DR.G128_CASES
FWD_SHAPES = SMALL + [s for kind, s in DR.G128_CASES if kind == "fwd"]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("family", DR.FAMILIES)
@pytest.mark.parametrize("kind,shape", PASS_CASES, ids=case_id)
def test_the_float32_chain_passes_the_comparator(kind, shape, family):
    m, i, o = shape
    x, w, bias, dy, _ = DR.operands(family, DR.seed_of(shape), m, i, o)
    acc = None
    for with_bias, relu in ((True, True), (False, False)) if kind == "fwd" else ((False, False),):
        a, b, f64, mag, k = DR.pass_problem(kind, x, w, bias, dy, with_bias, relu)
        acc = DR.chain32(a, b) if acc is None else acc
        chain = DR.epilogue32(acc, bias if with_bias else None, relu)
        if family == "ints":
            assert np.array_equal(chain.astype(np.float64), f64)             # exact: any order of summation gives this
        e32 = DR.e32_of(chain, f64, mag)
        ratio = DR.check_elementwise(chain, f64, mag, k, int(with_bias), e32, "%s %s %s" % (kind, shape, family))
        assert ratio <= 1.0 and (family != "ints" or e32 == 0.0)
        # E32 itself stays inside the a-priori bound with room to spare: K u is a worst case, the chain's errors mostly cancel
        assert e32 <= (k + 1) * DR.U


def capped(shape):
    """The batch cut so that the case's float32 chains stay near a second in all; the errors below live in columns, k and the
    last rows, not in the batch size."""
    m, i, o = shape
    return max(4, min(m, int(4e7 // (i * o)))) if m > 4 else m, i, o


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=case_id)
def test_wrong_outputs_are_rejected_and_the_old_metric_lets_some_through(shape):
    m, i, o = capped(shape)
    tol = DR.old_tolerance(i)
    for family in DR.FAMILIES:
        x, w, bias, dy, marks = DR.operands(family, DR.seed_of(shape), m, i, o)
        a, b, f64, mag, k = DR.pass_problem("fwd", x, w, bias, dy, True, False)
        right = DR.epilogue32(DR.chain32(a, b), bias)
        e32 = DR.e32_of(right, f64, mag)
        assert DR.old_metric(right, f64) <= tol
        for name in DR.WRONG:
            wrong = DR.wrong_forward(name, x, w, bias, marks)
            if wrong is None or np.array_equal(wrong, right):                 # the shape has no room for this error / it changes nothing
                assert family == "ints" or min(m, o) < 4 or i < 8, (name, shape)
                continue
            old = DR.old_metric(wrong, f64)
            if family == "ints":
                rejected = not np.array_equal(wrong.astype(np.float64), f64)
            else:
                try:
                    DR.check_elementwise(wrong, f64, mag, k, 8, e32, name)       # (8 slab adds + the bias add allowed: still rejected)
                    rejected = False
                except AssertionError:
                    rejected = True
            print("WRONG %-20s %-6s %-14s per element: %s; old metric %.2e against %.2e: %s"
                  % (name, family, case_id((m, i, o)), "rejected" if rejected else "ACCEPTED", old, tol,
                     "LET THROUGH" if old <= tol else "caught"))
            assert rejected, (name, family, shape)
            if family == "reals" and (name == "bias_rolled" or (name == "quiet_column_last_k" and i >= 2048)):
                assert old <= tol, (name, shape, old, tol)


def test_int_bias_and_families_are_what_they_say():
    for n in (1, 2, 5, 33, 512, 1924):
        b = DR.int_bias(n, n)
        assert b.shape == (n,) and np.abs(b).max() <= 3 and (n < 2 or (b[1:] != b[:-1]).all())
    assert len(np.unique(DR.int_bias(3, 512))) == 7
    with pytest.raises(AssertionError):
        DR.ints(0, (2, 2), 2 ** 21)
    x, w, bias, dy, marks = DR.operands("reals", 5, 67, 31, 66)
    assert (w[:, marks["zero_col"]] == 0).all() and (x[marks["zero_row"]] == 0).all() and (x[marks["pos_row"]] >= 0).all()
    loud = np.abs(w).max(0)
    assert loud[marks["quiet_col"]] < 2.0 ** -9 * loud.max()
    assert np.abs(x[marks["quiet_row"]]).max() < 2.0 ** -9 * np.abs(x).max()
    # bf16x2 keeps 16 significant bits, by truncation
    t = DR.reals(1, (1000,))
    assert (np.abs(DR.bf16x2(t)) <= np.abs(t)).all() and np.abs(DR.bf16x2(t) - t).max() <= 2.0 ** -15 * np.abs(t).max()
