"""The GPU engine's choice of the Schur product and its PCG plan
(csrc/megba/gpu/schur_plan.hpp), driven through the bindings without a device:
the knob-to-path table with the probe launches it makes, the comparison of
the four timings, and the plan fields.  E(l, r) in the comments is
(lds_eligible, rc_eligible).
"""
import itertools

import pytest

from megba_amd import _core

P = _core.SchurPath
NAME = {"lds": P.Lds, "lds-recompute": P.LdsRecompute,
        "fused-etx": P.FusedEtx, "separate": P.Separate}
SMALL, LARGE = 1000, 300000  # local edges: below / above the tuning threshold
TIME = None                  # "time the candidates"

# (n_local_edges, knobs, (l, r), failing probes, path, probes made in order,
#  (lds, lds-recompute) still candidates = timed)
UNTIMED = [
    (SMALL, {}, (1, 1), {}, "fused-etx", [], (0, 0)),
    (SMALL, {"no_etxfuse": 1}, (1, 1), {}, "separate", [], (0, 0)),
    (SMALL, {"etxfuse": 1}, (1, 1), {}, "fused-etx", [], (0, 0)),
    (SMALL, {"schur_lds": 1}, (1, 1), {}, "lds", ["lds"], (1, 0)),
    (SMALL, {"schur_lds": 1}, (1, 1), {"lds_launches": 0}, "fused-etx",
     ["lds"], (0, 0)),
    (SMALL, {"schur_lds": 1, "no_etxfuse": 1}, (1, 1), {}, "lds", ["lds"],
     (1, 0)),
    (SMALL, {"schur_lds": 1, "no_etxfuse": 1}, (0, 0), {}, "separate", [],
     (0, 0)),
    (SMALL, {"schur_recompute": 1}, (1, 1), {}, "lds-recompute",
     ["lds-recompute"], (0, 1)),
    (SMALL, {"schur_recompute": 1}, (1, 0), {}, "fused-etx", [], (0, 0)),
    (SMALL, {"schur_recompute": 1}, (1, 1), {"rc_launches": 0}, "fused-etx",
     ["lds-recompute"], (0, 0)),
    (SMALL, {"schur_recompute": 1, "schur_lds": 1}, (1, 1), {},
     "lds-recompute", ["lds-recompute"], (1, 1)),
    (SMALL, {"schur_recompute": 1, "schur_lds": 1}, (1, 0), {}, "lds",
     ["lds"], (1, 0)),
    (SMALL, {"schur_recompute": 1, "no_etxfuse": 1}, (1, 1), {},
     "lds-recompute", ["lds-recompute"], (0, 1)),
    (LARGE, {}, (1, 1), {}, TIME, ["lds-recompute", "lds"], (1, 1)),
    (LARGE, {}, (0, 0), {}, TIME, [], (0, 0)),
    (LARGE, {"schur_lds": 1}, (1, 1), {}, "lds", ["lds"], (1, 0)),
    (LARGE, {"schur_lds": 1}, (0, 0), {}, "fused-etx", [], (0, 0)),
    (LARGE, {"no_etxfuse": 1}, (1, 1), {}, "separate", [], (0, 0)),
    # a candidate whose first launch the runtime refuses is not timed
    (LARGE, {}, (1, 1), {"lds_launches": 0}, TIME, ["lds-recompute", "lds"],
     (0, 1)),
    (LARGE, {}, (1, 1), {"rc_launches": 0}, TIME, ["lds-recompute", "lds"],
     (1, 0)),
]


@pytest.mark.parametrize("n_l,knobs,elig,probe_fail,path,probes,timed",
                         UNTIMED)
def test_untimed_decision(n_l, knobs, elig, probe_fail, path, probes, timed):
    got = _core.schur_path_untimed(
        n_l, bool(elig[0]), bool(elig[1]),
        **{k: bool(v) for k, v in {**knobs, **probe_fail}.items()})
    assert got[0] == (NAME[path] if path else None)
    assert got[1] == [NAME[p] for p in probes]
    # where the decision is left to the timings, these are timed next to the
    # two two-pass paths
    assert got[2:] == tuple(bool(t) for t in timed)


def test_tuning_threshold():
    assert _core.schur_path_untimed(199999, True, True)[0] == P.FusedEtx
    assert _core.schur_path_untimed(200000, True, True)[0] is TIME


# ms [fused-etx, separate, lds, lds-recompute]; None = not timed
TIMINGS = [
    ([2, 3, 1, 0.5], "lds-recompute"),
    ([2, 3, 1, 1.5], "lds"),
    ([2, 3, 2.5, 1.5], "lds-recompute"),
    ([2, 3, 2.5, 2.2], "fused-etx"),
    ([3, 2, 2.5, 2.2], "separate"),
    ([2, 2, None, None], "fused-etx"),
    ([2, 3, 2, None], "fused-etx"),   # a tie is not a win
    ([2, 3, 1, 1], "lds"),            # a tie is not a win
    ([2, 3, None, 1.9], "lds-recompute"),
]


@pytest.mark.parametrize("ms,path", TIMINGS)
def test_decision_from_timings(ms, path):
    # the engine leaves an untimed entry at 0 ms, which must not win
    got = _core.schur_path_from_timings(
        [0.0 if t is None else t for t in ms], ms[2] is not None,
        ms[3] is not None)
    assert got == NAME[path]


def test_plan_fields():
    for tuned, implicit, n_long, noop, fused, no_pcg_fuse in itertools.product(
            NAME.values(), (False, True), (0, 2), (False, True),
            (False, True), (False, True)):
        path, rotated, reads_pad, merge = _core.pcg_plan(
            tuned, implicit, n_long, noop, fused=fused,
            no_pcg_fuse=no_pcg_fuse)
        # MEGBA_FUSED replaces the product; the tuner's path is still what
        # the engine reports
        assert path == (P.OnePass if fused else tuned)
        assert rotated == (not no_pcg_fuse)
        assert reads_pad == (implicit or path != P.Separate)
        assert merge == (path in (P.Lds, P.LdsRecompute) and rotated
                         and n_long == 0 and noop)


def test_plan_literal_rows():
    # (tuned, implicit, n_long_pts, allreduce_is_noop, knobs) ->
    # (path, rotatedBody, productReadsPad, mergeReduceBApply)
    rows = [
        ((P.Lds, True, 0, True, {}), (P.Lds, True, True, True)),
        ((P.LdsRecompute, True, 0, True, {}),
         (P.LdsRecompute, True, True, True)),
        ((P.Lds, True, 2, True, {}), (P.Lds, True, True, False)),
        ((P.Lds, True, 0, False, {}), (P.Lds, True, True, False)),
        ((P.Lds, True, 0, True, {"no_pcg_fuse": True}),
         (P.Lds, False, True, False)),
        ((P.FusedEtx, True, 0, True, {}), (P.FusedEtx, True, True, False)),
        ((P.Separate, False, 0, True, {}), (P.Separate, True, False, False)),
        ((P.Separate, True, 0, True, {}), (P.Separate, True, True, False)),
        ((P.FusedEtx, False, 0, True, {}), (P.FusedEtx, True, True, False)),
        ((P.Lds, True, 0, True, {"fused": True}),
         (P.OnePass, True, True, False)),
        ((P.Separate, False, 0, True, {"fused": True}),
         (P.OnePass, True, True, False)),
    ]
    for (tuned, implicit, n_long, noop, knobs), plan in rows:
        assert _core.pcg_plan(tuned, implicit, n_long, noop, **knobs) == plan


def test_path_names():
    for name, path in NAME.items():
        assert _core.schur_path_name(path) == name
