"""CPU-only: the float64 reference tests/test_gpu_wgrad_ops.py judges the weight-gradient launches by (tests/_wgrad_np.py) is
itself checked -- against torch.autograd of an explicit conv over the materialised crop + concat at every shape the GPU tests
launch, against a triple loop at the two smallest shapes, and for reading nothing outside the windows."""
import numpy as np
import pytest

import _wgrad_np as W

SHAPES = W.all_shapes()
IDS = [i for i, _ in SHAPES]


def _close(got, want, tol=1e-12):
    return np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("shape", [s for _, s in SHAPES], ids=IDS)
def test_reference_equals_autograd_of_the_materialised_conv(shape):
    x0, x1, dzs = W.make_inputs(shape, seed=5)
    dw, db = W.reference(x0, x1, dzs, shape["K"], shape["parts"])
    aw, ab = W.reference_autograd(x0, x1, dzs, shape["K"], shape["parts"])
    assert dw.shape == (shape["K"], shape["C0"] + shape["C1"], shape["N"]) and db.shape == (shape["N"],)
    assert np.abs(dw).max() < 1e3 and np.abs(db).max() < 1e3          # nothing of the 1e4 fill came in
    assert _close(dw, aw) and _close(db, ab)


def test_reference_equals_the_triple_loop_at_the_smallest_shapes():
    size = lambda s: s["B"] * (s["C0"] + s["C1"]) * s["N"] * s["K"] * sum(p["Tq"] for p in s["parts"])
    small = sorted(SHAPES, key=lambda e: size(e[1]))[:2]
    assert len({i for i, _ in small}) == 2
    for _, shape in small:
        x0, x1, dzs = W.make_inputs(shape, seed=6)
        dw, db = W.reference(x0, x1, dzs, shape["K"], shape["parts"])
        lw, lb = W.reference_loops(x0, x1, dzs, shape["K"], shape["parts"])
        assert _close(dw, lw) and _close(db, lb)
    # ... and at a tiny two-part, two-source, shifted shape that the loops finish quickly (both loaders)
    tiny = W.make_shape(2, 3, 2, 4, 5, [dict(loader=1, x0_off=2, x1_off=1, Tin=21, Tq=9),
                                          dict(loader=0, x0_off=0, x1_off=0, Tin=12, shift=2, Tq=12)])
    x0, x1, dzs = W.make_inputs(tiny, seed=7)
    dw, db = W.reference(x0, x1, dzs, 5, tiny["parts"])
    lw, lb = W.reference_loops(x0, x1, dzs, 5, tiny["parts"])
    aw, ab = W.reference_autograd(x0, x1, dzs, 5, tiny["parts"])
    assert _close(dw, lw) and _close(db, lb) and _close(dw, aw) and _close(db, ab)


@pytest.mark.parametrize("shape", [s for _, s in SHAPES], ids=IDS)
def test_elements_outside_the_windows_do_not_change_the_result(shape):
    x0, x1, dzs = W.make_inputs(shape, seed=8)
    y0, y1, dys = W.refill_outside(shape, x0, x1, dzs, seed=9)
    changed = int((x0 != y0).sum()) + sum(int((a != b).sum()) for a, b in zip(dzs, dys))
    assert changed > 0                                                 # there IS something outside every window
    dw, db = W.reference(x0, x1, dzs, shape["K"], shape["parts"])
    ew, eb = W.reference(y0, y1, dys, shape["K"], shape["parts"])
    assert np.array_equal(dw, ew) and np.array_equal(db, eb)


def test_inputs_put_the_fill_everywhere_but_the_windows():
    shape = W.up_shape(*W.UP_MAIN, 5, 2)
    x0, x1, dzs = W.make_inputs(shape, seed=1)
    p = shape["parts"][0]
    for rows, off in ((x0, p["x0_off"]), (x1, p["x1_off"])):
        inside = np.zeros(rows.shape[2], dtype=bool)
        inside[off:off + p["Tin"]] = True
        assert np.abs(rows[:, :, inside]).max() <= 1.0 and np.abs(rows[:, :, ~inside]).min() >= 0.5 * W.FILL
        assert np.isfinite(rows).all()
    assert np.abs(dzs[0][:, :, :p["Tq"]]).max() <= 1.0 and np.abs(dzs[0][:, :, p["Tq"]:]).min() >= 0.5 * W.FILL
    b = W.make_inputs(shape, seed=1, bf16_x0=True, bf16_x1=True, bf16_dz=True)
    assert np.array_equal(W.bf16_round(b[0]), b[0]) and np.abs(b[0] - x0).max() <= 2.0 ** -8 * W.FILL * 1.5
