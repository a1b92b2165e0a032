"""The memory-state cases of pp_project_set: dirty outputs, poisoned and reused scratch, a used context after a refused call,
every leg held to the bits of the base leg (pp_project_set promises identical reruns and is not in REFERENCE_BOUND_ONLY).

The case table (tests/memory_state_cases.py) and its runner (tests/test_memory_state.py) are left as they are.  This module
builds its four cases as the table's own Case records, runs each through the runner's unchanged test_memory_state, and
puts them into M.CASES so that the runner's coverage test finds pp_project_set covered.  Nothing here depends on the order
in which pytest imports the modules: the runner is imported first, so its own parametrisation holds the table as committed,
and M.CASES is then REBOUND to a longer list rather than appended to.  The one thing a new module cannot do is be imported
when tests/test_memory_state.py is run on its own: its coverage test then reports pp_project_set as neither a case nor
exempt; the same check is test_every_entry_point_is_covered below.

Inputs, comparison and restatement are those of tests/test_projection.py (test_kernel_equals_members): every plane is the
restated reduction of the member resampled alone, bit for bit.  Cases: image + labels (std, the second walk), labels only,
the median's select, five views with five labels."""
import ctypes as C

import numpy as np
import pytest

from tests import memory_state_cases as M
from tests import test_memory_state as runner
from tests import test_projection as PJ


def _projection(sid, axis, kind, nlabels, with_image, nviews):
    shape = (9, 17, 33)
    grid = PJ.grid_named("oblique", shape)
    img, labs = PJ.volumes(shape, nlabels, 90 + nlabels)
    img = img if with_image else None
    views = PJ.standard_views(grid)[:nviews]
    linterp = [PJ.NEAR if k % 2 == 0 else PJ.LIN for k in range(nlabels)]

    def run(leg):
        gi, gl = PJ.run_fused(leg, img, labs, grid, axis, views, kind, PJ.LIN, linterp)
        res = {f"label{k}": o for k, o in enumerate(gl)}
        if with_image:
            res["image"] = gi
        return res

    def check(leg, outs):
        vi, vl = PJ.resample_members(leg, img, labs, grid, views, PJ.LIN, linterp)
        for v in range(nviews):
            if with_image:
                PJ.assert_plane(outs["image"][v], vi[v], kind, axis, f"memory-state project_set view {v}")
            for k in range(nlabels):
                np.testing.assert_array_equal(outs[f"label{k}"][v], PJ.PR.label_max(vl[k][v], axis))

    def bad(leg):       # no views
        g = grid.geom()
        return leg.lib.pp_project_set(leg.ctx.h, C.byref(g), axis, None, 1, leg.p(PJ.volumes(shape, 0, 1)[0]), 0, PJ.LIN, 0.0, None, None, None,
                                      0, None)

    return M.Case(id=f"project-set-{sid}", fns=("pp_project_set",), run=run, check=check, nvox=int(np.prod(shape)) * nviews,
                  family="resample", bad=bad)


CASES = [_projection("image-labels", 0, "std", 3, True, 1), _projection("labels-only", 1, "max", 2, False, 1),
         _projection("median", 0, "median", 0, True, 1), _projection("multi-view", 2, "mean", 5, True, 5)]
if not any(c.id == CASES[0].id for c in M.CASES):
    M.CASES = M.CASES + CASES        # a new list: the runner's parametrisation keeps the table as committed


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_memory_state_of_project_set(backend, monkeypatch, case):
    runner.test_memory_state(backend, monkeypatch, case)


def test_every_entry_point_is_covered():
    assert {c.id for c in CASES} <= {c.id for c in M.CASES}
    runner.test_every_entry_point_is_a_case_or_exempt_for_a_reason()
