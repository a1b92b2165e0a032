"""The memory-state cases of the SIFT entry points (csrc/pp_sift.h): dirty outputs, poisoned and reused scratch, a used
context after a refused call, every leg held to the bits of the base leg (all four promise identical reruns; none is in
REFERENCE_BOUND_ONLY).

As in tests/test_memory_radiomics.py the case table and its runner are left as they are: this module builds M.Case records,
runs each through the runner's unchanged test_memory_state and REBINDS M.CASES to a longer list, so that the runner's coverage
test finds the four functions covered.  test_stream_legs_of_sift runs the cases through the unchanged delayed-stream and
busy-default legs of tests/test_stream_order.py.

Inputs, references and bounds are those of tests/test_sift.py.  Cases: the extremum pass on both sides of its 32 x 8 tile,
the descriptors (clamped windows and a constant level), the match with and without the gate (63 rows against 65: more than
one row block, a partial column tile), the points (oblique direction cosines, points outside the field)."""
import ctypes as C

import numpy as np
import pytest

from tests import memory_state_cases as M
from tests import test_memory_projection  # noqa: F401  (their cases join M.CASES too: the coverage test holds when this module runs alone)
from tests import test_memory_radiomics  # noqa: F401
from tests import test_memory_state as runner
from tests import test_sift as TS

RR = TS.RR


def _extrema(name):
    stack = TS.gaussian_stack(name)

    def run(leg):
        cand, _ = TS.reference_keypoints(name)
        rc, count, index, values = TS.run_extrema(leg, stack, len(cand))
        assert rc == 0
        return {"count": np.array([count]), "index": index[:count], "values": values[:count]}

    def check(leg, outs):               # test_keypoints_equal_the_restatement
        cand, fit = TS.reference_keypoints(name)
        want = np.flatnonzero(fit["keep"])
        assert outs["count"][0] == len(want) and np.array_equal(outs["index"], cand[want])
        bound = TS.offset_bound(fit)[want]
        assert np.all(np.abs(outs["values"][:, :3] - fit["offset"][want]) <= bound[:, None])
        assert np.all(np.abs(outs["values"][:, 3] - fit["response"][want]) <= fit["gnorm"][want] * bound + 8 * TS.U * np.abs(fit["response"][want]))

    def bad(leg):
        return TS.run_extrema(leg, stack, 4, value_range=-1.0)[0]

    return M.Case(id=f"sift-extrema-{name}", fns=("pp_dog_extrema_f32",), run=run, check=check, nvox=stack.size, family="sift", bad=bad)


def _describe(name):
    stack, spacing, kp = TS.descriptor_input(name)

    def run(leg):
        rc, desc = TS.run_describe(leg, stack, spacing, kp)
        assert rc == 0
        return {"descriptors": leg.host(desc)}

    def check(leg, outs):               # test_descriptors_against_the_restatement
        for k, (x, y, z, l) in enumerate(kp):
            want, marked = RR.descriptor(stack[l], spacing, (x, y, z))
            assert not marked
            assert np.all(np.abs(outs["descriptors"][k].astype(np.float64) - want.astype(np.float64)) <= 2.0 ** -23)

    def bad(leg):
        outside = kp.copy()
        outside[0, 3] = stack.shape[0]
        return TS.run_describe(leg, stack, spacing, outside)[0]

    return M.Case(id=f"sift-describe-{name}", fns=("pp_sift_describe_f32",), run=run, check=check, nvox=stack.size, family="sift", bad=bad)


def _match(gate):
    a, b, pa, pb = TS.match_input(63, 65, 768)
    radius = 6.0 if gate else None

    def run(leg):
        rc, idx, best, second = TS.run_match(leg, a, b, *((pa, pb, radius) if gate else ()))
        assert rc == 0
        return {"index": leg.host(idx), "best": leg.host(best), "second": leg.host(second)}

    def check(leg, outs):               # test_matching_against_fp64
        TS.check_match(a, b, pa, pb, radius, outs["index"], outs["best"], outs["second"])

    def bad(leg):
        return TS.run_match(leg, a, b, pa, None, 1.0)[0]

    return M.Case(id=f"sift-match-{'gated' if gate else 'all'}", fns=("pp_descriptor_match_f32",), run=run, check=check, nvox=a.size + b.size,
                  family="sift", bad=bad)


def _points(direction_name):
    field, D, pts, c, n_inside = TS.points_input(direction_name)
    size = M.size_of(TS.FIELD_SHAPE)

    def call(leg, f):
        from platipy_amd import _lib

        out = leg.hempty(pts.shape, np.float64)
        geom = _lib.make_geom(size, TS.FIELD_SPACING, TS.FIELD_ORIGIN, D.ravel())
        rc = leg.lib.pp_transform_points_f64(leg.ctx.h, f, C.byref(geom), M.hptr(np.ascontiguousarray(pts)), len(pts), M.hptr(out))
        return rc, out

    def run(leg):
        rc, out = call(leg, leg.p(field))
        assert rc == 0
        return {"points": out}

    def check(leg, outs):               # test_points_through_a_field
        want, scale = RR.transform_points(field, size, TS.FIELD_SPACING, TS.FIELD_ORIGIN, D.ravel(), pts)
        assert np.all(np.abs(outs["points"] - want).max(axis=1) <= TS.point_bound(c, pts, scale))
        assert np.array_equal(outs["points"][n_inside:], pts[n_inside:])

    def bad(leg):
        return call(leg, None)[0]

    return M.Case(id=f"sift-points-{direction_name}", fns=("pp_transform_points_f64",), run=run, check=check, nvox=field.size, family="sift", bad=bad)


CASES = [_extrema("below-tile"), _extrema("above-tile"), _extrema("19x21x37"), _describe("20x22x24"), _match(False), _match(True), _points("rot")]
if not any(c.id == CASES[0].id for c in M.CASES):
    M.CASES = M.CASES + CASES        # a new list: the runner's parametrisation keeps the table as committed


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_memory_state_of_sift(backend, monkeypatch, case):
    runner.test_memory_state(backend, monkeypatch, case)


def test_every_entry_point_is_covered():
    assert {c.id for c in CASES} <= {c.id for c in M.CASES}
    assert {fn for c in CASES for fn in c.fns} == {"pp_dog_extrema_f32", "pp_sift_describe_f32", "pp_descriptor_match_f32", "pp_transform_points_f64"}
    assert not ({fn for c in CASES for fn in c.fns} & set(runner.REFERENCE_BOUND_ONLY))
    runner.test_every_entry_point_is_a_case_or_exempt_for_a_reason()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stream_legs_of_sift(gpu_backend, monkeypatch, case):
    """The delayed-stream and busy-default legs of tests/test_stream_order.py, two passes each, on these cases."""
    from tests import test_stream_order as SOT

    SOT.test_stream_legs(gpu_backend, monkeypatch, case)
