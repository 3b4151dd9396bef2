"""The serving plan's MLP and tree entries without a GPU: ``build_plan(..., nonlinear=True)``
eligibility, the launcher's validation of the two kinds, and the CPU mirror
(csrc/host/serve_plan_cpu.cpp) against ``Pipeline.predict`` — 40 points per case, the cases
and seeds of the GPU tests (tests/serving_plan_nonlinear_cases.py). Tree answers are equal
on every row; NN scores within rtol 1e-4 / atol 1e-3, NN classes and ±1 equal on every row
that is no near-tie (at most 2 of those, by the reference's own forward pass).

The mirror also runs stand-alone under AddressSanitizer + UBSan on hostile tree arenas
(csrc/tests/serve_plan_selftest.cpp): no Python in that process, nothing preloaded.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from omldm_amd.ops import serving as S
from tests import serving_plan_nonlinear_cases as NL
from tests.serving_plan_cases import N_POINTS, compare, make_pipeline, payload, points, space_small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", NL.CASES)
def test_mirror_equals_pipeline_predict(case):
    sp = NL.space_of(case)
    batch = points(sp)
    assert batch.B == N_POINTS
    pipe = NL.make(1, case, sp, "cpu", batch)
    assert S.build_plan([pipe], sp).served == [], "left direct without the flag"
    plan = S.build_plan([pipe], sp, nonlinear=True)
    assert plan.served == [(1, 0)] and not plan.direct
    assert int(plan.table[0, S.PL_KIND]) == (4 if case in NL.NN_CASES else 5)
    got = NL.mirror(plan, NL.arena_of(plan), sp, batch)[:, 0]
    want, tie = NL.reference(pipe, batch)
    compare(pipe, got, want, tie, case)
    if case in NL.HT_CASES:
        assert not tie.any() and torch.equal(got, want)


def test_old_and_new_kinds_in_one_plan():
    """Both parameter sets of the GPU bank test: every output of the mixed plan equals its
    single-entry plan's output and the reference (their seeds stay within the tie cap)."""
    from tests.serving_plan_cases import reference as linear_reference

    sp = space_small(True)
    batch = points(sp)
    for shift in (0, 200):
        pipes = NL.mixed(sp, batch, "cpu", shift)
        plan = S.build_plan(pipes, sp, nonlinear=True)
        assert plan.served == [(10 + i, i) for i in range(len(NL.MIXED))]
        ends = 0
        for _, off, n in plan.regions:  # the regions tile the arena without overlap
            assert off == ends
            ends = off + n
        assert ends == plan.arena_floats
        got = NL.mirror(plan, NL.arena_of(plan), sp, batch)
        for i, pipe in enumerate(pipes):
            one = S.build_plan([pipe], sp, nonlinear=True)
            alone = NL.mirror(one, NL.arena_of(one), sp, batch)[:, 0]
            assert torch.equal(got[:, i], alone), NL.MIXED[i]
            ref = linear_reference if NL.MIXED[i] in NL.OLD else NL.reference
            want, tie = ref(pipe, batch)
            compare(pipe, got[:, i], want, tie, f"set {shift} {NL.MIXED[i]}")


def test_tree_cases_are_what_they_claim():
    """The shapes the cases are there for: the tie leaf is reached and answers its lowest
    top class; the chain's last leaf sits at maxDepth and is reached; the deeper tree's walk
    ends on an inner node; the large tree uses ≥ 1000 of 1024 nodes; the tree behind
    PolynomialFeatures splits only on features ≥ 5."""
    sp = space_small(True)
    batch = points(sp)

    def routed(name):
        pipe = NL.make(1, name, sp, "cpu", batch)
        L = pipe.learner
        return L, L._route(pipe._pre(batch, False).num.float())

    L, leaf = routed("ht_fresh")
    assert int(L.nnodes) == 1 and bool((leaf == 0).all()) and float(L.cc.sum()) == 0.0
    L, leaf = routed("ht_complete63")
    assert int(L.nnodes) == 63 and L.Cn == 3
    row = L.cc[leaf[0]]
    assert float(row[1]) == float(row[2]) == float(row.max()) and float(row[0]) < float(row[1])
    assert float(L.cc[leaf[0]].argmax()) == 1.0
    L, leaf = routed("ht_chain_at_max_depth")
    last = 2 * L.depth  # depth = its index / 2
    assert int(L.nnodes) == last + 1 and float(L.feat[last]) < 0 and bool((leaf == last).any())
    L, leaf = routed("ht_deeper_than_max_depth")
    stop = 2 * (L.depth + 1)  # the inner node at depth maxDepth + 1
    assert float(L.feat[stop]) >= 0 and bool((leaf == stop).any())
    assert int(leaf.max()) <= stop
    L, leaf = routed("ht_1024_nodes_32_classes")
    assert L.N == 1024 and L.Cn == 32 and int(L.nnodes) >= 1000
    assert len(set(leaf.tolist())) > 10
    L, leaf = routed("ht_poly_high_features")
    assert L.d == 20 and float(L.feat[L.feat >= 0].min()) >= 5
    assert len(set(leaf.tolist())) > 1
    # 104 features do not fit the lanes: a lazy poly2 stage, splits on products and inputs
    spw = NL.space_of("ht_std_poly_104_features")
    bw = points(spw)
    pipe = NL.make(1, "ht_std_poly_104_features", spw, "cpu", bw)
    L = pipe.learner
    used = L.feat[L.feat >= 0]
    assert L.d == 104 and float(used.max()) >= 64 and float(used.min()) < 13
    plan = S.build_plan([pipe], spw, nonlinear=True)
    e = plan.table[0]
    assert int(e[S.PL_STAGES]) == 2 and list(e[S.PL_STAGE0 + 4:S.PL_STAGE0 + 8]) == [2, 0, 0, 13]
    assert len(set(L._route(pipe._pre(bw, False).num.float()).tolist())) > 5
    # only a tree, and only behind the map as its last stage, takes it lazily
    for other in (("NN", {"hiddenLayers": [8]}, ["PolynomialFeatures"], {}),
                  ("K-means", {"k": 3}, ["PolynomialFeatures"], {}),
                  ("HT", {"nClasses": 2}, ["PolynomialFeatures", "StandardScaler"], {})):
        p = make_pipeline(2, other, spw, "cpu", 1)
        assert S.build_plan([p], spw, nonlinear=True).direct == [p], other
    p = make_pipeline(2, ("HT", {"nClasses": 2}, ["PolynomialFeatures"], {}), spw, "cpu", 1)
    assert S.build_plan([p], spw, nonlinear=True).served == [(2, 0)]
    assert S.build_plan([p], spw).direct == [p]


def test_what_the_wave_cannot_serve_is_left_direct():
    sp = space_small(True)
    for i, name in enumerate(NL.LEFT_DIRECT):
        pipe = NL.make_direct(1 + i, name, sp, "cpu")
        plan = S.build_plan([pipe], sp, nonlinear=True)
        assert plan.served == [] and plan.direct == [pipe], name
    # the limits themselves are served
    edge = [make_pipeline(1, ("NN", {"hiddenLayers": [64, 64, 64], "nClasses": 64}, [], {}), sp,
                          "cpu", 1),
            make_pipeline(2, ("HT", {"nClasses": 32, "maxNodes": 1024}, [], {}), sp, "cpu", 1)]
    assert S.build_plan(edge, sp, nonlinear=True).served == [(1, 0), (2, 1)]
    # nonlinear=False (the default): every NN and tree is left direct, every other case served
    batch = points(sp)
    pipes = [NL.make(1 + i, c, sp, "cpu", batch) for i, c in enumerate(NL.CASES)]
    pipes.append(make_pipeline(40, "svm_std", sp, "cpu", 1))
    plan = S.build_plan(pipes, sp)
    assert plan.served == [(40, 0)] and plan.direct == pipes[:-1]
    assert S.build_plan(pipes, sp, nonlinear=False).served == [(40, 0)]


def test_publish_layout():
    """``serving_write``: per layer the transposed weight block then the bias; the tree's
    region is the head of its state vector."""
    sp = space_small(True)
    batch = points(sp)
    pipe = NL.make(1, "nn_bin_tanh_std", sp, "cpu", batch)
    plan = S.build_plan([pipe], sp, nonlinear=True)
    arena = NL.arena_of(plan)
    e = plan.table[0]
    assert list(e[S.PL_AUX:S.PL_AUX + 7]) == [3, 1, 1, 5, 64, 3, 1]
    L = pipe.learner
    assert int(e[S.PL_WIDTH]) == L.flat.numel() == 5 * 64 + 64 + 64 * 3 + 3 + 3 + 1
    o, src = int(e[S.PL_OFF]), 0
    for a, b in zip(L.widths[:-1], L.widths[1:]):
        W = L.flat[src:src + a * b].view(b, a)
        assert torch.equal(arena[o:o + a * b].view(a, b), W.t())
        assert torch.equal(arena[o + a * b:o + a * b + b], L.flat[src + a * b:src + a * b + b])
        o, src = o + a * b + b, src + a * b + b
    pipe = NL.make(2, "ht_complete63", sp, "cpu", batch)
    plan = S.build_plan([pipe], sp, nonlinear=True)
    arena = NL.arena_of(plan)
    L = pipe.learner
    assert list(plan.table[0, S.PL_AUX:S.PL_AUX + 3]) == [L.N, 3, L.depth]
    assert plan.arena_floats == L.N * 7 and torch.equal(arena, L.state[: L.N * 7])


def test_launcher_validation_refuses_bad_entries():
    sp = space_small(True)
    batch = points(sp)
    num, cat = payload(batch, 0)
    nn = NL.make(1, "nn_reg_relu", sp, "cpu", batch)
    ht = NL.make(2, "ht_complete63", sp, "cpu", batch)
    for pipe, bad in ((nn, [(0, 0), (0, 5), (1, 4), (2, 3), (3, 65), (4, 65), (4, 0), (3, 4)]),
                      (ht, [(0, 0), (0, 1025), (1, 33), (1, 1), (2, -1)])):
        plan = S.build_plan([pipe], sp, nonlinear=True)
        arena = NL.arena_of(plan)
        S.cpu_serve_plan(plan.table, arena, sp, num, cat)
        for word, value in bad:  # L = 0, a width of 65, w_0 ≠ D, N = 0, C = 33, …
            t = plan.table.copy()
            t[0, S.PL_AUX + word] = value
            with pytest.raises(ValueError, match="-10"):
                S.cpu_serve_plan(t, arena, sp, num, cat)
        with pytest.raises(ValueError, match="-13"):  # the region ends one float past the arena
            S.cpu_serve_plan(plan.table, arena[:-1], sp, num, cat)
        t = plan.table.copy()
        t[0, S.PL_OFF] = 1
        with pytest.raises(ValueError, match="-13"):
            S.cpu_serve_plan(t, arena, sp, num, cat)
        t = plan.table.copy()
        t[0, S.PL_KIND] = 3  # still no kind
        with pytest.raises(ValueError, match="-10"):
            S.cpu_serve_plan(t, arena, sp, num, cat)
    assert plan.table.dtype == np.int32
    # a lazy poly2 stage: only as the last stage of a tree entry
    spw = NL.space_of("ht_std_poly_104_features")
    bw = points(spw)
    num, cat = payload(bw, 0)
    pipe = NL.make(1, "ht_std_poly_104_features", spw, "cpu", bw)
    plan = S.build_plan([pipe], spw, nonlinear=True)
    arena = NL.arena_of(plan)
    S.cpu_serve_plan(plan.table, arena, spw, num, cat)
    t = plan.table.copy()
    t[0, S.PL_STAGE0:S.PL_STAGE0 + 8] = np.roll(t[0, S.PL_STAGE0:S.PL_STAGE0 + 8], 4)
    with pytest.raises(ValueError, match="-12"):  # lazy first, the scaler after it
        S.cpu_serve_plan(t, arena, spw, num, cat)
    t = plan.table.copy()
    t[0, S.PL_STAGE0 + 7] = 12  # on another width
    with pytest.raises(ValueError, match="-12"):
        S.cpu_serve_plan(t, arena, spw, num, cat)
    t = plan.table.copy()
    t[0, S.PL_KIND], t[0, S.PL_WIDTH] = 2, 13  # a k-means entry behind it
    with pytest.raises(ValueError, match="-12"):
        S.cpu_serve_plan(t, arena, spw, num, cat)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_mirror_selftest_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "serve_plan_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "csrc", "host"),
           os.path.join(ROOT, "csrc", "host", "serve_plan_cpu.cpp"),
           os.path.join(ROOT, "csrc", "tests", "serve_plan_selftest.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives
    # (the program then does not depend on its place in the library list)
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "serve plan selftest OK" in r.stdout
