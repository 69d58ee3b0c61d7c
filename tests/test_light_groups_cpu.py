"""Host logic of the light workgroup groups, without a GPU: sdsm_solve_class at the limits of the light layout (through sdsm_plan_solve_classes, which
calls it for every candidate of a plan with given setup results)."""
import ctypes as C

import numpy as np

from superdsm_amd.testing import plan_of_squares as _plan_of_squares
from test_capi_cpu import _schedule

CLS_1, CLS_1B, CLS_2, CLS_2B, CLS_3, CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT = range(8)
KL_NMAX, KL_EMAX = 288, 12400          # SDSM_KL_NMAX, SDSM_KL_EMAX


def _classes(lib, plan, n, status, M, env):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a = [np.full(n, v, np.int32) for v in (status, M, env)]
    cls = np.full(n, -9, np.int32)
    assert lib.sdsm_plan_solve_classes(plan, p(a[0]), p(a[1]), p(a[2]), p(cls)) == 0
    return cls


def test_solve_class_at_the_limits_of_the_light_layout():
    from superdsm_amd import _capi
    lib = _capi.lib()
    sides = [30] * 1100 + [100] * 6 + [180] * 2                 # throughput mode: groups for the regions above 8192 pixels; more than 1024 candidates: light groups by default
    n = len(sides)
    plan = _plan_of_squares(sides)
    try:
        g, _ = _schedule(plan, n, 0)
        grouped = g > 0
        assert grouped.sum() == 8
        M = KL_NMAX - 6
        at = _classes(lib, plan, n, 0, M, KL_EMAX)               # 6 + M and the envelope equal to the limits
        assert (at[grouped] == CLS_WIDE_LIGHT).all() and (at[~grouped] == CLS_2B).all()
        assert (_classes(lib, plan, n, 0, M, KL_EMAX + 1)[grouped] == CLS_WIDE2B).all()       # one above: the layout of class 2b, on the other side queue
        assert (_classes(lib, plan, n, 0, M + 1, KL_EMAX)[grouped] == CLS_WIDE2B).all()
        assert (_classes(lib, plan, n, 0, M + 1, 21)[grouped] == CLS_WIDE2B).all() and (_classes(lib, plan, n, 0, 0, 0)[grouped] == CLS_WIDE_LIGHT).all()
        assert (_classes(lib, plan, n, 0, 512 - 6, 15170)[grouped] == CLS_WIDE2B).all() and (_classes(lib, plan, n, 0, 512 - 5, 11000)[grouped] == CLS_WIDE).all()
        assert (_classes(lib, plan, n, 0, M, 15171)[grouped] == CLS_3).all()                  # no group layout holds it
        assert (_classes(lib, plan, n, 3, M, 100) == -1).all()
        # the classes of single workgroups do not move
        assert (_classes(lib, plan, n, 0, 100, 2560)[~grouped] == CLS_1).all() and (_classes(lib, plan, n, 0, 100, 2561)[~grouped] == CLS_1B).all()
        # a smaller limit (diagnostic entry point), none at all (the two layouts in their earlier order), more than the layout holds
        assert lib.sdsm_set_light_envelope_limit(5000) == 0
        assert (_classes(lib, plan, n, 0, M, 5000)[grouped] == CLS_WIDE_LIGHT).all() and (_classes(lib, plan, n, 0, M, 5001)[grouped] == CLS_WIDE2B).all()
        assert lib.sdsm_set_light_envelope_limit(0) == 0
        assert (_classes(lib, plan, n, 0, M, 5000)[grouped] == CLS_WIDE).all() and (_classes(lib, plan, n, 0, M, 11001)[grouped] == CLS_WIDE2B).all()
        assert lib.sdsm_set_light_envelope_limit(KL_EMAX + 1) == -1 and b'12400' in lib.sdsm_last_error()
        # a plan of at most 1024 candidates has light groups only on request (every class-1 candidate has a slot at once there)
        small = _plan_of_squares([30] * 200 + [100] * 6 + [180] * 2)
        try:
            gs, _ = _schedule(small, 208, 0)
            assert lib.sdsm_set_light_envelope_limit(-1) == 0
            assert (_classes(lib, small, 208, 0, M, 5000)[gs > 0] == CLS_WIDE).all()
            assert lib.sdsm_set_light_envelope_limit(KL_EMAX) == 0
            assert (_classes(lib, small, 208, 0, M, 5000)[gs > 0] == CLS_WIDE_LIGHT).all()
        finally:
            lib.sdsm_plan_destroy(small)
        # mode 2: no groups, no group classes
        _schedule(plan, n, 2)
        assert lib.sdsm_set_light_envelope_limit(-1) == 0
        assert not np.isin(_classes(lib, plan, n, 0, M, 5000), (CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT)).any()
    finally:
        lib.sdsm_set_light_envelope_limit(-1)
        lib.sdsm_plan_destroy(plan)


def _base_members(N, grouped):
    """One member per 8192 pixels, 2 .. 8 (layout_plan before the bonus)."""
    return np.where(grouped, np.clip(-(-N // 8192), 2, 8), 0)


def test_member_bonus_goes_to_the_largest_regions_that_may_not_be_light():
    """layout_plan, throughput mode, on fake candidate tables (squares; grid spacing 8: the bound on M is ceil(side / 8)^2, so a square of side >= 129 may
    exceed the 288 unknowns of the light class): one member more for the grouped regions that may not be light and have at least 90 % of the pixels of the
    largest grouped region, inside the budget of 256 members and the 8 members of a group."""
    from superdsm_amd import _capi
    lib = _capi.lib()
    # (a) the two largest (32 400 px, bound 529) get a fifth member; 30 625 px (94 %) too; 19 600 px (60 %, bound 324) and 10 000 px (bound 169: light) do not
    sides = [30] * 200 + [100] * 6 + [140] * 3 + [175] + [180] * 2
    n, N = len(sides), np.array(sides) ** 2
    plan = _plan_of_squares(sides)
    g, _ = _schedule(plan, n, 0)
    assert g[N == 32400].tolist() == [5, 5] and g[N == 30625].tolist() == [5] and g[N == 19600].tolist() == [3] * 3 and g[N == 10000].tolist() == [2] * 6 and (g[N == 900] == 0).all()
    g1, _ = _schedule(plan, n, 1)                                # latency mode: no bonus
    assert g1[N == 32400].tolist() == [4, 4] and g1[N == 30625].tolist() == [4]
    lib.sdsm_plan_destroy(plan)
    # (b) a region large enough to be light by its bound never gets one, however large it is next to the others: 128 x 128 (bound 256) among smaller ones
    sides = [30] * 200 + [128] * 2 + [100] * 4
    n, N = len(sides), np.array(sides) ** 2
    plan = _plan_of_squares(sides)
    g, _ = _schedule(plan, n, 0)
    assert g[N == 16384].tolist() == [2, 2] and g[N == 10000].tolist() == [2] * 4
    lib.sdsm_plan_destroy(plan)
    # (c) at most 8 members: 67 600 px already has them
    sides = [30] * 400 + [260] + [250]
    n, N = len(sides), np.array(sides) ** 2
    plan = _plan_of_squares(sides)
    g, _ = _schedule(plan, n, 0)
    assert g[N == 67600].tolist() == [8] and g[N == 62500].tolist() == [8]
    lib.sdsm_plan_destroy(plan)
    # (d) the budget of 256 members holds, and what is left of it goes to the largest first
    sides = list(range(120, 220)) + [100] * 100
    n, N = len(sides), np.array(sides) ** 2
    plan = _plan_of_squares(sides)
    g, _ = _schedule(plan, n, 0)
    base = _base_members(N, g > 0)
    extra = g - base
    eligible = (g > 0) & (N * 100 >= N[g > 0].max() * 90) & (np.ceil(np.array(sides) / 8) ** 2 > 282)
    assert g.sum() <= 256 and g.max() <= 8 and set(extra.tolist()) <= {0, 1} and not extra[~eligible].any()
    assert extra.sum() == min(eligible.sum(), 256 - base.sum())
    got = np.sort(N[extra > 0])[::-1]
    assert (got == np.sort(N[eligible])[::-1][:len(got)]).all()
    lib.sdsm_plan_destroy(plan)
    # (e) a plan without groups stays without (the synthetic 4096^2 plan)
    sides = [70] * 8000 + [120] * 40 + [135] * 2
    plan = _plan_of_squares(sides)
    g, _ = _schedule(plan, len(sides), 0)
    assert (g == 0).all()
    lib.sdsm_plan_destroy(plan)
