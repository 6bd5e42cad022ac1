"""Row-scaled error of a kernel's rows against a reference's, for the tolerance tests.

Only rows that are non-finite in the REFERENCE are left out (a reference row whose magnitude
exceeds 1e30 counts as non-finite: it is about to overflow, and its last bits decide which side
does first).  A row that is finite in the reference and non-finite in the kernel is an error.
``min_share``: the share of the reference's rows that must be compared -- every comparison
after more than one step or epoch demands 0.9, so that it cannot pass on inf / NaN rows alone."""
import numpy as np

BIG = 1e30


def finite_rows(b):
    b = np.asarray(b, np.float64)
    b = b.reshape(b.shape[0], -1)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(b) & (np.abs(b) <= BIG), axis=1)


def rel(a, b, min_share=0.0):
    """max over the reference's finite rows of max|a - b| / (max|b| + 1e-6); inf when ``a`` is not
    finite in such a row.  Asserts that at least ``min_share`` of the rows are compared."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    assert a.shape == b.shape
    ok = finite_rows(b)
    share = float(ok.mean()) if ok.size else 1.0
    assert share >= min_share, f"only {share:.0%} of the reference rows are finite (need {min_share:.0%})"
    if not ok.any():
        return 0.0
    a, b = a[ok], b[ok]
    if not np.all(np.isfinite(a)):
        return float("inf")
    return float(np.max(np.abs(a - b) / (np.max(np.abs(b), axis=1, keepdims=True) + 1e-6)))
