"""``audiolcm_amd.windows``: the one weight table and the one validator behind ``pipeline.joint_weights`` and
``pipeline.ring_weights``, and the module's independence of torch and of the HIP library.  No GPU."""
import subprocess
import sys

import numpy as np
import pytest

import test_joint_host as line
import test_loop_host as ring
from conftest import REPO

# (L, W, overlap) of line plans with more than one window
LINE_PLANS = [c for c in line.CASES if c[0] > c[1]] + [(845, 312, 156), (73, 15, 7)]


def _line_starts(L, W, overlap):
    from audiolcm_amd.windows import long_windows
    spans, w = long_windows(L, W, overlap)
    assert w == W and len(spans) >= 2
    return [s for s, _ in spans]


@pytest.mark.parametrize("L,W,overlap", LINE_PLANS)
def test_a_line_plan_has_one_table_in_both_forms(L, W, overlap):
    from audiolcm_amd.windows import window_weights
    starts = _line_starts(L, W, overlap)
    on_line, on_ring = window_weights(starts, W, L, overlap), window_weights(starts, W, L, overlap, ring=True)
    assert np.array_equal(on_ring, on_line) and on_ring is not on_line


@pytest.mark.parametrize("L,W,overlap", line.CASES)
def test_window_weights_on_a_line(L, W, overlap):
    from audiolcm_amd.pipeline import joint_weights
    from audiolcm_amd.windows import window_weights
    starts = line._starts(L, W, overlap)
    wn = window_weights(starts, W, L, overlap)
    assert wn.dtype == np.float32 and np.array_equal(wn, line._restated(starts, W, L, overlap)[0].astype(np.float32))
    assert joint_weights(starts, W, L, overlap) is wn and not wn.flags.writeable


@pytest.mark.parametrize("args", [a for a, _ in ring.PLANS])
def test_window_weights_on_a_ring(args):
    from audiolcm_amd.pipeline import ring_weights
    from audiolcm_amd.windows import loop_windows, window_weights
    L = args[0]
    starts, W, overlap = loop_windows(L, args[1], args[2])
    wn = window_weights(starts, W, L, overlap, ring=True)
    assert wn.dtype == np.float32 and np.array_equal(wn, ring._restated(starts, W, L, overlap)[0].astype(np.float32))
    assert ring_weights(starts, W, L, overlap) is wn and not wn.flags.writeable


def _params(test):
    """The argument rows of a parametrised test."""
    return [m.args[1] for m in test.pytestmark if m.name == "parametrize"][0]


@pytest.mark.parametrize("starts,W,L,overlap", _params(line.test_joint_weights_refuses))
def test_line_plans_refused(starts, W, L, overlap):
    from audiolcm_amd.windows import window_weights
    with pytest.raises(ValueError):
        window_weights(starts, W, L, overlap, ring=False)


@pytest.mark.parametrize("starts,W,L,overlap", _params(ring.test_ring_weights_refuses))
def test_ring_plans_refused(starts, W, L, overlap):
    from audiolcm_amd.windows import window_weights
    with pytest.raises(ValueError):
        window_weights(starts, W, L, overlap, ring=True)


def test_the_rows_that_separate_line_and_ring():
    from audiolcm_amd.windows import window_weights
    for ring_form in (False, True):                                    # the last window neither ends at L nor reaches it
        with pytest.raises(ValueError):
            window_weights([0, 20], 40, 61, 20, ring=ring_form)
    assert window_weights([0, 20], 40, 50, 20, ring=True).shape == (2, 40)   # past the end: a ring wraps, a line cannot
    with pytest.raises(ValueError):
        window_weights([0, 20], 40, 50, 20, ring=False)
    assert window_weights([0], 40, 40, 20, ring=False).shape == (1, 40)      # one window is a line, and closes no ring
    with pytest.raises(ValueError):
        window_weights([0], 40, 40, 20, ring=True)
    with pytest.raises(ValueError, match="32"):
        window_weights(list(range(33)), 40, 72, 20)


def test_region_window_limit():
    from audiolcm_amd.windows import JOINT_MAX_WINDOWS, check_region_windows
    check_region_windows(0, 660, JOINT_MAX_WINDOWS, 40)
    with pytest.raises(ValueError, match="32"):
        check_region_windows(0, 680, JOINT_MAX_WINDOWS + 1, 40)


def test_windows_module_needs_neither_torch_nor_the_library():
    code = ("import sys; import audiolcm_amd.windows; "
            "print([m for m in ('torch', 'audiolcm_amd._hip') if m in sys.modules])")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "[]"
