"""``--forecastServer plans``: the engine's per-record lane on the plan-driven wave
(engine/forecast_server.py, csrc/kernels/serving.hip: serve_plan_kernel).

* scaled, ORR, MultiClassPA and K-means pipelines are answered by the resident wave
  (``_served``), NN and Hoeffding trees by one-row predicts (``_direct``);
* every answer equals the batched predict of the same pipeline (scores within rtol 1e-4 /
  atol 1e-3, clusters exactly, ±1 and classes on every row that is no near-tie);
* a publish republishes scaler and model parameters;
* a job whose pipelines are all plan-served runs the native lane on file topics;
* Delete reconfigures the plan; ``close`` ends the wave.

Geometry of tests/test_forecast_server_gpu.py. Without the feature ``plans`` is no
recognised flag value: the job has no forecast server and these tests fail.
"""
import json
import os
import uuid

import pytest
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.engine.job import Job
from omldm_amd.io.parse import parse_records
from omldm_amd.io.synthetic import synth_json_records
from omldm_amd.io.transport import FileBroker, MemoryBroker
from omldm_amd.parallel.comm import Comm
from omldm_amd.utils.config import JobConfig
from tests.serving_plan_cases import compare, reference

pytestmark = pytest.mark.gpu

SP = FeatureSpace(13, 0, 26, 1 << 18)
TOPICS = ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
          "predictionsAddr", "performanceAddr")


def _args(addr):
    args = []
    for k in TOPICS:
        args += [f"--{k}", addr]
    return args + ["--hashDim", str(SP.dim), "--batchSize", "2000", "--timeout", "300",
                   "--parallelism", "8", "--forecastServer", "plans"]


def _memory_job():
    name = uuid.uuid4().hex
    cfg = JobConfig.from_args(_args(f"memory://{name}"))
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    return Job(cfg, Comm(), "cuda"), br


def _file_job(root):
    cfg = JobConfig.from_args(_args(f"file://{root}"))
    br = FileBroker(root)
    for t in ("trainingData", "forecastingData", "requests", "predictions", "responses",
              "performance"):
        br.create_topic(t, 2 if t in ("trainingData", "forecastingData") else 1)
    return Job(cfg, Comm(), "cuda"), br


def _create(br, pid, name, hyper=None, pre=None):
    br.produce("requests", json.dumps({
        "id": pid, "request": "Create",
        "learner": {"name": name, "hyperParameters": hyper or {}},
        "preProcessors": [{"name": p} for p in (pre or [])],
        "trainingConfiguration": {"protocol": "Synchronous"}}))


def _moved(records):
    """The same records drawn elsewhere and labelled the other way round: training on
    them moves scaler moments, centroids and weights."""
    out = []
    for r in records:
        d = json.loads(r)
        d["numericalFeatures"] = [3.0 * v + 2.0 for v in d["numericalFeatures"]]
        d["target"] = -d["target"]
        out.append(json.dumps(d))
    return out


def _three_classes(records):
    """Targets 0 / 1 / 2 by the first numerical feature (a MultiClassPA of K = 3)."""
    out = []
    for r in records:
        d = json.loads(r)
        x = d["numericalFeatures"][0]
        d["target"] = 0.0 if x < -0.4 else (1.0 if x < 0.4 else 2.0)
        out.append(json.dumps(d))
    return out


def _rounds_done(job):
    """Waits for the ticks' rounds and their publish copy. A tick does not wait for its own
    round, and the lane adopts a publish only once its copy has completed: until then an
    answer comes from the bank before it (engine/forecast_server.py, "at most one round
    stale"), and these tests compare with the model after the last round. As
    tests/test_forecast_server_gpu.py does after its ticks — on the ticks' stream, not the
    device: the resident wave runs there."""
    (job.lanes.compute if job.lanes is not None else torch.cuda.current_stream()).synchronize()


def _check(job, pids, fc, preds):
    """Each pipeline's answers, in record order, against its batched predict."""
    batch, _, _ = parse_records(fc, job.space)
    batch = batch.without_raw()
    got = {}
    for pid in pids:
        mine = [p for p in preds if p["mlpId"] == pid]
        assert [p["dataPoint"] for p in mine] == [json.loads(r) for r in fc], pid
        got[pid] = torch.tensor([p["prediction"] for p in mine], dtype=torch.float32)
        want, tie = reference(job.pipes[pid], batch)
        compare(job.pipes[pid], got[pid], want, tie,
                f"pipeline {pid} {job.pipes[pid].learner.NAME}")
    return got


SEVEN = [(1, "SVM", None, None), (2, "SVM", None, ["StandardScaler"]),
         (3, "NN", {"hiddenLayers": [8]}, None), (4, "ORR", None, ["MinMaxScaler"]),
         (5, "MultiClassPA", {"nClasses": 2}, None), (6, "K-means", {"k": 3}, None),
         (7, "HT", {"nClasses": 2}, ["PolynomialFeatures"])]


def test_plans_serve_every_kind_publish_and_reconfigure():
    job, br = _memory_job()
    assert job.fserver is not None and job.fserver.plans
    fs = job.fserver
    try:
        for pid, name, hyper, pre in SEVEN:
            _create(br, pid, name, hyper, pre)
        for r in synth_json_records(6000, SP):
            br.produce("trainingData", r)
        for _ in range(4):
            job.tick()
        _rounds_done(job)
        assert fs.serving and [pid for pid, _, _ in fs._served] == [1, 2, 4, 5, 6]
        assert [pid for pid, _ in fs._direct] == [3, 7]
        assert not fs.native  # in-process topics keep the Python lane
        fc = synth_json_records(12, SP, start=70000, operation="forecasting")
        for r in fc:
            br.produce("forecastingData", r)
        job.tick()
        assert not fs.fallback and fs.served == 12
        preds = [json.loads(x) for x in br.records("predictions")]
        assert sorted(p["mlpId"] for p in preds) == sorted(list(range(1, 8)) * 12)
        first = _check(job, range(1, 8), fc, preds)
        fam = fs.family_percentiles()
        assert set(fam) >= {"SVM", "ORR", "MultiClassPA", "K-means", "NN", "HT"}, fam

        # publish: two more ticks of training move the scaler and the models; the same
        # records are answered from the republished parameters
        for r in _moved(synth_json_records(4000, SP, start=20000)):
            br.produce("trainingData", r)
        for _ in range(2):
            job.tick()
        _rounds_done(job)
        n0 = len(preds)
        for r in fc:
            br.produce("forecastingData", r)
        job.tick()
        preds = [json.loads(x) for x in br.records("predictions")][n0:]
        assert len(preds) == 84
        second = _check(job, (2, 6), fc, preds)
        for pid in (2, 6):
            assert not torch.equal(second[pid], first[pid]), (pid, first[pid], second[pid])

        # a Delete of one served pipeline reconfigures the plan; the rest keep being answered
        br.produce("requests", json.dumps({"id": 5, "request": "Delete"}))
        job.tick()
        assert [pid for pid, _, _ in fs._served] == [1, 2, 4, 6]
        assert [pid for pid, _ in fs._direct] == [3, 7]
        n0 += len(preds)
        for r in fc[:4]:
            br.produce("forecastingData", r)
        job.tick()
        preds = [json.loads(x) for x in br.records("predictions")][n0:]
        assert sorted(p["mlpId"] for p in preds) == sorted([1, 2, 3, 4, 6, 7] * 4)
        _check(job, (1, 2, 4, 6), fc[:4], preds)

        # close ends the wave
        srv = fs._server
        assert srv is not None and srv.lib.omldm_serve_alive(srv.mb) == 1
        stream = srv.stream
        fs.close()
        assert fs._server is None and srv.mb is None and stream.query()
    finally:
        fs.close()


def test_plans_run_the_native_lane_on_file_topics(tmp_path):
    job, br = _file_job(str(tmp_path))
    fs = job.fserver
    try:
        _create(br, 1, "SVM", None, ["StandardScaler"])
        _create(br, 2, "MultiClassPA", {"nClasses": 3})
        _create(br, 3, "K-means", {"k": 3})
        for r in _three_classes(synth_json_records(6000, SP)):
            br.produce("trainingData", r)
        for _ in range(4):
            job.tick()
        _rounds_done(job)
        assert fs.serving and [pid for pid, _, _ in fs._served] == [1, 2, 3]
        assert not fs._direct
        assert fs.native, "every pipeline plan-served + file topics: the native lane"
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
        # one line per pipeline and record, the pipelines of a record together and in order
        assert [p["mlpId"] for p in preds] == [1, 2, 3] * 12
        for k in range(12):
            assert preds[3 * k]["dataPoint"] == preds[3 * k + 1]["dataPoint"] == \
                preds[3 * k + 2]["dataPoint"]
        # (the lane reads the two forecasting partitions in turn: compare in its order)
        order = [json.dumps(preds[3 * k]["dataPoint"], sort_keys=True) for k in range(12)]
        by_point = {json.dumps(json.loads(r), sort_keys=True): r for r in fc}
        assert sorted(order) == sorted(by_point)
        _check(job, (1, 2, 3), [by_point[o] for o in order], preds)
        assert fs.native_stats()["served"] == 12
    finally:
        job.close()
