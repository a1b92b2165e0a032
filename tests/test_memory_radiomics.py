"""The memory-state cases of the radiomics entry points (csrc/pp_radiomics.h): dirty outputs, poisoned and reused scratch, a
used context after a refused call, every leg held to the bits of the base leg (all four promise identical reruns; none is in
REFERENCE_BOUND_ONLY).

As in tests/test_memory_projection.py the case table and its runner are left as they are: this module builds M.Case records,
runs each through the runner's unchanged test_memory_state and REBINDS M.CASES to a longer list, so that the runner's coverage
test finds the four functions covered.  test_stream_legs_of_radiomics runs the cases through the unchanged delayed-stream
and busy-default legs of tests/test_stream_order.py.  (That module takes list(M.CASES) when it is imported; in a run of the
whole suite that is after this module, so its own parametrisation and its neighbours test hold these cases as well.)

Inputs, references and bounds are those of tests/test_radiomics.py: tables equal the brute-force restatement, the moments
lie within the bound derived there.  Cases: the moments (all values; a range about a centre), the discretisation (aligned),
the neighbourhood tables from LDS (Ng = 19, one GLCM group), in thirteen GLCM groups (Ng = 79) and with global atomics
(Ng = 102), the runs from LDS and with global atomics."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import memory_state_cases as M
from tests import test_memory_projection  # noqa: F401  (its cases join M.CASES too: the coverage test holds when this module runs alone)
from tests import test_memory_state as runner
from tests import test_radiomics as TR

U = 2.0 ** -53


def _moments(name):
    img, mask, _ = TR.case_input(name)
    v = img[mask != 0].astype(np.float64)
    ranges = ((-np.inf, np.inf, float(v.mean())), (float(np.percentile(v, 10)), float(np.percentile(v, 90)), 3.5))

    def run(leg):
        out = {}
        for k, (lo, hi, c) in enumerate(ranges):
            count, sums = leg.hempty(1, np.int64), leg.hempty(6, np.float64)
            assert leg.lib.pp_masked_moments_f32(leg.ctx.h, leg.p(img), leg.p(mask), img.size, lo, hi, c, M.hptr(count, C.c_int64), M.hptr(sums)) == 0
            out[f"count{k}"], out[f"sums{k}"] = count, sums
        return out

    def check(leg, outs):               # test_moments_against_fp64
        for k, (lo, hi, c) in enumerate(ranges):
            sel = v[(v >= lo) & (v <= hi)]
            d = sel - c
            assert outs[f"count{k}"][0] == sel.size
            for j, terms in enumerate([d, np.abs(d), d ** 2, d ** 3, d ** 4, sel ** 2]):
                assert abs(outs[f"sums{k}"][j] - math.fsum(terms.tolist())) <= (sel.size + 8) * U * math.fsum(np.abs(terms).tolist())

    def bad(leg):
        count, sums = leg.hempty(1, np.int64), leg.hempty(6, np.float64)
        return leg.lib.pp_masked_moments_f32(leg.ctx.h, None, leg.p(mask), img.size, 0.0, 1.0, 0.0, M.hptr(count, C.c_int64), M.hptr(sums))

    return M.Case(id=f"radiomics-moments-{name}", fns=("pp_masked_moments_f32",), run=run, check=check, nvox=img.size, family="reduce", bad=bad)


def _discretise(name):
    img, mask, bw = TR.case_input(name)

    def run(leg):
        rc, lev = TR.discretise(leg, img, mask, TR.RR.bin_edges(img[mask != 0], bw))
        assert rc == 0
        return {"levels": leg.host(lev).view(np.uint16)}

    def check(leg, outs):               # test_tables_equal_the_restatement
        assert np.array_equal(outs["levels"].reshape(img.shape), TR.reference_tables(name)["levels"])

    def bad(leg):
        return TR.discretise(leg, img, mask, [0.0, 1.0, 1.0])[0]

    return M.Case(id=f"radiomics-discretise-{name}", fns=("pp_radiomics_discretise_f32",), run=run, check=check, nvox=img.size, family="reduce",
                  bad=bad)


def _texture(name, which):
    img, mask, _ = TR.case_input(name)
    size = M.size_of(img.shape)
    p = lambda a: M.hptr(a, C.c_int64)  # noqa: E731
    ref = lambda: TR.reference_tables(name)  # noqa: E731  (made when a leg first runs, not when the module is collected)

    def run(leg):
        lev8, ng = ref()["levels"].view(np.uint8), ref()["ng"]
        sz = (C.c_int * 3)(*size)
        if which == "runs":
            glrlm = leg.hempty((13, ng, max(img.shape)), np.int64)
            assert leg.lib.pp_texture_runs_u16(leg.ctx.h, leg.p(lev8), sz, ng, max(img.shape), p(glrlm)) == 0
            return {"glrlm": glrlm}
        glcm, gldm = leg.hempty((13, ng, ng), np.int64), leg.hempty((ng, 27), np.int64)
        nn, ns = leg.hempty((ng, 27), np.int64), leg.hempty((ng, 27), np.int64)
        assert leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, leg.p(lev8), sz, ng, p(glcm), p(gldm), p(nn), p(ns)) == 0
        return {"glcm": glcm, "gldm": gldm, "ngtdm_n": nn, "ngtdm_s": ns}

    def check(leg, outs):               # test_tables_equal_the_restatement
        for k, got in outs.items():
            assert np.array_equal(got + got.transpose(0, 2, 1) if k == "glcm" else got, ref()[k]), k

    def bad(leg):
        ng = ref()["ng"]
        sz = (C.c_int * 3)(*size)
        out = leg.hempty((13, ng, max(max(img.shape), ng)), np.int64)
        if which == "runs":
            return leg.lib.pp_texture_runs_u16(leg.ctx.h, None, sz, ng, max(img.shape), p(out))
        return leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, None, sz, ng, p(out), None, None, None)

    fn = "pp_texture_runs_u16" if which == "runs" else "pp_texture_neighbourhood_u16"
    return M.Case(id=f"radiomics-{which}-{name}", fns=(fn,), run=run, check=check, nvox=img.size, family="reduce", bad=bad)


CASES = [_moments("noise-19x21x37-faces"), _discretise("noise-19x21x37-faces"), _texture("noise-19x21x37-faces", "neighbourhood"),
         _texture("ng-79", "neighbourhood"), _texture("ng-102", "neighbourhood"), _texture("noise-19x21x37-faces", "runs"),
         _texture("ng-79", "runs")]
if not any(c.id == CASES[0].id for c in M.CASES):
    M.CASES = M.CASES + CASES        # a new list: the runner's parametrisation keeps the table as committed


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_memory_state_of_radiomics(backend, monkeypatch, case):
    runner.test_memory_state(backend, monkeypatch, case)


def test_every_entry_point_is_covered():
    assert {c.id for c in CASES} <= {c.id for c in M.CASES}
    assert {fn for c in CASES for fn in c.fns} == {"pp_masked_moments_f32", "pp_radiomics_discretise_f32", "pp_texture_neighbourhood_u16",
                                                   "pp_texture_runs_u16"}
    assert not ({fn for c in CASES for fn in c.fns} & set(runner.REFERENCE_BOUND_ONLY))
    runner.test_every_entry_point_is_a_case_or_exempt_for_a_reason()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stream_legs_of_radiomics(gpu_backend, monkeypatch, case):
    """The delayed-stream and busy-default legs of tests/test_stream_order.py, two passes each, on these cases."""
    from tests import test_stream_order as SOT

    SOT.test_stream_legs(gpu_backend, monkeypatch, case)
