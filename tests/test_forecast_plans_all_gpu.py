"""``--forecastServer plans-all``: NN and Hoeffding-tree pipelines on the plan-driven wave as
well (engine/forecast_server.py; csrc/kernels/serving.hip: serve_plan_kernel<true>).

* the seven pipelines of tests/test_forecast_plans_gpu.py (``SEVEN``) are all answered by
  the resident wave (``_served`` 1..7, ``_direct`` empty); every answer equals the batched predict of the
  same pipeline (the rules of tests/test_forecast_plans_gpu.py; a tree's answers on every
  row);
* a publish republishes the NN's weights and the tree;
* an ``Update`` of the NN's activation (a word of its plan entry) reconfigures the plan;
* Delete reconfigures the plan; ``close`` ends the wave;
* a job with an NN and an HT pipeline runs the native lane on file topics. Without the
  feature ``plans-all`` is no recognised flag value and such a job keeps the Python lane:
  these tests fail.

Pipeline 7 of ``SEVEN`` is an HT behind PolynomialFeatures(2) over 13 numerical features:
104 dense values, more than the wave's 64 lanes. A tree reads one feature per node, so its
plan entry takes the map as a lazy stage (the product of two lanes per node) and is served.
"""
import gc
import json
import os

import pytest
import torch

from tests.serving_plan_cases import compare
from tests.serving_plan_nonlinear_cases import reference as nl_reference
from tests.test_forecast_plans_gpu import (SEVEN, SP, _check, _create, _file_job, _memory_job,
                                           _moved, _rounds_done)
from omldm_amd.io.parse import parse_records
from omldm_amd.io.synthetic import synth_json_records

pytestmark = pytest.mark.gpu


@pytest.fixture
def plans_all(monkeypatch):
    """The jobs of tests/test_forecast_plans_gpu.py under ``--forecastServer plans-all``."""
    import tests.test_forecast_plans_gpu as base

    args = base._args
    monkeypatch.setattr(base, "_args", lambda addr: [
        "plans-all" if a == "plans" else a for a in args(addr)])


def _check_nl(job, pids, fc, preds):
    """``_check`` for NN and HT pipelines: the near-ties of the NN's own forward pass; a
    tree's answers equal on every row."""
    batch, _, _ = parse_records(fc, job.space)
    batch = batch.without_raw()
    got = {}
    for pid in pids:
        mine = [p for p in preds if p["mlpId"] == pid]
        assert [p["dataPoint"] for p in mine] == [json.loads(r) for r in fc], pid
        got[pid] = torch.tensor([p["prediction"] for p in mine], dtype=torch.float32)
        want, tie = nl_reference(job.pipes[pid], batch)
        compare(job.pipes[pid], got[pid], want, tie,
                f"pipeline {pid} {job.pipes[pid].learner.NAME}")
        if job.pipes[pid].learner.NAME == "HT":
            assert torch.equal(got[pid], want)
    return got


def test_plans_all_serves_every_learner_publish_update_and_reconfigure(plans_all):
    job, br = _memory_job()
    fs = job.fserver
    assert fs is not None and fs.plans and fs.nonlinear
    try:
        for pid, name, hyper, pre in SEVEN:
            _create(br, pid, name, hyper, pre)
        for r in synth_json_records(6000, SP):
            br.produce("trainingData", r)
        for _ in range(4):
            job.tick()
        _rounds_done(job)
        assert fs.serving and [pid for pid, _, _ in fs._served] == [1, 2, 3, 4, 5, 6, 7]
        assert fs._direct == []
        assert int(fs._plan.table[6, 8 + 0]) == 2, "the tree's PolynomialFeatures: a lazy stage"
        assert not fs.native  # in-process topics keep the Python lane
        print("tree nodes in use:", int(job.pipes[7].learner.nnodes.item()))
        fc = synth_json_records(12, SP, start=70000, operation="forecasting")

        def ask(recs):
            n0 = len(br.records("predictions"))
            for r in recs:
                br.produce("forecastingData", r)
            job.tick()
            return [json.loads(x) for x in br.records("predictions")][n0:]

        preds = ask(fc)
        assert not fs.fallback and fs.served == 12
        assert sorted(p["mlpId"] for p in preds) == sorted(list(range(1, 8)) * 12)
        _check(job, (1, 2, 4, 5, 6), fc, preds)
        first = _check_nl(job, (3, 7), fc, preds)
        assert set(fs.family_percentiles()) >= {"SVM", "ORR", "MultiClassPA", "K-means", "NN",
                                                "HT"}

        # publish: more training moves the NN's weights and the tree's counts; the same
        # records are answered from the republished models
        flat0 = job.pipes[3].learner.flat.clone()
        tree0 = job.pipes[7].learner.state[: job.pipes[7].learner.N * 6].clone()
        for r in _moved(synth_json_records(4000, SP, start=20000)):
            br.produce("trainingData", r)
        for _ in range(2):
            job.tick()
        _rounds_done(job)
        assert not torch.equal(flat0, job.pipes[3].learner.flat)
        assert not torch.equal(tree0, job.pipes[7].learner.state[: tree0.numel()])
        preds = ask(fc)
        assert len(preds) == 84
        _check(job, (2, 6), fc, preds)
        _check_nl(job, (3, 7), fc, preds)

        # an Update of the NN's activation: a word of its plan entry, so the plan is rebuilt
        assert int(fs._plan.table[2, 25]) == 0  # relu
        br.produce("requests", json.dumps({
            "id": 3, "request": "Update",
            "learner": {"name": "NN", "hyperParameters": {"activation": "tanh"}}}))
        job.tick()
        assert job.pipes[3].learner.act_name == "tanh"
        assert [pid for pid, _, _ in fs._served] == [1, 2, 3, 4, 5, 6, 7]
        assert int(fs._plan.table[2, 25]) == 1
        preds = ask(fc)
        _check_nl(job, (3, 7), fc, preds)  # (the reference: the forward pass under tanh)
        del first

        # a Delete of one served pipeline reconfigures the plan; the rest keep being answered
        br.produce("requests", json.dumps({"id": 5, "request": "Delete"}))
        job.tick()
        assert [pid for pid, _, _ in fs._served] == [1, 2, 3, 4, 6, 7]
        assert fs._direct == []
        preds = ask(fc[:4])
        assert sorted(p["mlpId"] for p in preds) == sorted([1, 2, 3, 4, 6, 7] * 4)
        _check(job, (1, 2, 4, 6), fc[:4], preds)
        _check_nl(job, (3, 7), fc[:4], preds)

        # close ends the wave
        srv = fs._server
        assert srv is not None and srv.lib.omldm_serve_alive(srv.mb) == 1
        stream = srv.stream
        fs.close()
        assert fs._server is None and srv.mb is None and stream.query()
    finally:
        fs.close()
        job.close()
        del job, fs
        gc.collect()  # the job's streams, events and pinned buffers are freed here, not later


def test_plans_all_runs_the_native_lane_with_nn_and_ht(plans_all, tmp_path):
    job, br = _file_job(str(tmp_path))
    fs = job.fserver
    try:
        _create(br, 1, "SVM", None, ["StandardScaler"])
        _create(br, 2, "NN", {"hiddenLayers": [8]})
        _create(br, 3, "HT", {"nClasses": 2})
        for r in synth_json_records(6000, SP):
            br.produce("trainingData", r)
        for _ in range(4):
            job.tick()
        _rounds_done(job)
        assert fs.serving and [pid for pid, _, _ in fs._served] == [1, 2, 3]
        assert not fs._direct
        assert fs.native, "NN and HT plan-served + file topics: the native lane"
        fc = synth_json_records(12, SP, start=70000, operation="forecasting")
        for r in fc:
            br.produce("forecastingData", r)
        assert fs.catch_up(10.0)
        preds = []
        d = os.path.join(br.root, "predictions")
        for f in sorted(os.listdir(d)):
            with open(os.path.join(d, f), "rb") as fh:
                preds += [json.loads(x) for x in fh.read().splitlines() if x.strip()]
        assert len(preds) == 36
        assert [p["mlpId"] for p in preds] == [1, 2, 3] * 12
        # (the lane reads the two forecasting partitions in turn: compare in its order)
        order = [json.dumps(preds[3 * k]["dataPoint"], sort_keys=True) for k in range(12)]
        by_point = {json.dumps(json.loads(r), sort_keys=True): r for r in fc}
        assert sorted(order) == sorted(by_point)
        recs = [by_point[o] for o in order]
        _check(job, (1,), recs, preds)
        _check_nl(job, (2, 3), recs, preds)
        assert fs.native_stats()["served"] == 12
    finally:
        job.close()
        del job, fs
        gc.collect()
