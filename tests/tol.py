"""Float comparisons of the GPU tests with their measured error on record.

north_star asks for "within 1e-5 relative" on float outputs.  Two readings are measured for every comparison that goes
through `check_close`: the max-norm error (largest |got - want| over the largest |want|) and the element-relative error over
the entries that are not small (|want| > floor * max|want|; below that an fp32 result carries cancellation noise relative to
the LARGE terms it was summed from, not to itself).  With DEFTET_TOLERANCE_REPORT=<file.jsonl> every call appends its two
measured values, so that the asserted bounds can be kept at a small multiple of what the hardware actually delivers
(profiles/r05_tolerances.json is such a run at the BASELINE sizes).
"""
import json
import os

import numpy as np


def _np64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def check_close(name, got, want, maxnorm, elem_rel=None, floor=1e-3, mask=None):
    got, want = _np64(got), _np64(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if mask is not None:
        m = np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask, dtype=bool)
        got, want = got[m], want[m]
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(got - want)
    mn = float(err.max() / scale) if scale > 0 else float(err.max() if err.size else 0.0)
    big = np.abs(want) > floor * scale
    er = float((err[big] / np.abs(want[big])).max()) if big.any() else 0.0
    path = os.environ.get("DEFTET_TOLERANCE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"name": name, "n": int(want.size), "scale": scale, "maxnorm_err": mn, "elem_rel_err": er,
                                "elem_rel_floor": floor, "asserted_maxnorm": maxnorm, "asserted_elem_rel": elem_rel}) + "\n")
    assert mn <= maxnorm, "%s: max-norm error %.3g > %.3g" % (name, mn, maxnorm)
    if elem_rel is not None:
        assert er <= elem_rel, "%s: element-relative error %.3g > %.3g (entries above %g of the maximum)" % (name, er, elem_rel, floor)
    return mn, er


def check_bound(name, got, want, bound, mask=None):
    """Error over a per-element bound: |got - want| <= bound entry by entry (bound broadcasts against want; where it is zero the
    entries must be equal).  Reports and returns the worst ratio error / bound."""
    got, want = _np64(got), _np64(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bound = np.broadcast_to(_np64(bound), want.shape)
    if mask is not None:
        m = np.broadcast_to(np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask, dtype=bool), want.shape)
        got, want, bound = got[m], want[m], bound[m]
    assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound >= 0).all(), name
    err = np.abs(got - want)
    err = np.where(np.isfinite(err), err, np.inf)                    # a NaN where a number is due is an error of any size
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    path = os.environ.get("DEFTET_TOLERANCE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"name": name, "n": int(want.size), "scale": float(np.abs(want).max()) if want.size else 0.0,
                                "max_err": float(err.max()) if err.size else 0.0, "worst_err_over_bound": worst,
                                "asserted_err_over_bound": 1.0}) + "\n")
    assert worst <= 1.0, "%s: error is %.3g of its bound at the worst of %d entries (%d above)" % (name, worst, want.size, int((ratio > 1).sum()))
    return worst
