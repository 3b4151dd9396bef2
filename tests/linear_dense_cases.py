"""Shared by the dense-round tests: a Job on the MemoryBroker fed numerical-only records
(``--catFeatures 0``), as tests/test_matrix.py::_run drives one."""
from __future__ import annotations

import json
import uuid

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.engine.job import Job
from omldm_amd.io.synthetic import synth_json_records
from omldm_amd.io.transport import MemoryBroker
from omldm_amd.parallel.comm import Comm
from omldm_amd.utils.config import JobConfig

DIM = 1 << 16


def run_job(pipes, field_aware: bool, device, n: int = 1200, ticks: int = 4, task: int = 0):
    """``pipes``: [(id, learner name, hyper-parameters, preprocessor or None)]. Trains them
    on ``n`` synthetic records with 5 numerical and no categorical features and returns
    {id: (weights, running totals)} as CPU tensors."""
    name = uuid.uuid4().hex
    addr = f"memory://{name}"
    args = []
    for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
              "predictionsAddr", "performanceAddr"):
        args += [f"--{k}", addr]
    args += ["--hashDim", str(DIM), "--batchSize", "400", "--timeout", "200",
             "--parallelism", "4", "--numFeatures", "5", "--catFeatures", "0",
             "--fieldAware", str(field_aware).lower()]
    cfg = JobConfig.from_args(args)
    sp = FeatureSpace(5, 0, 0, DIM, field_aware=field_aware)
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    job = Job(cfg, Comm(), device)
    try:
        for pid, learner, hyper, pre in pipes:
            br.produce("requests", json.dumps({
                "id": pid, "request": "Create",
                "learner": {"name": learner, "hyperParameters": hyper or {}},
                "preProcessors": [{"name": pre}] if pre else [],
                "trainingConfiguration": {"protocol": "Synchronous"}}))
        for r in synth_json_records(n, sp, task=task):
            br.produce("trainingData", r)
        for _ in range(ticks):
            job.tick()
        out = {}
        for pid, *_ in pipes:
            assert pid in job.pipes
            lr = job.pipes[pid].learner
            lr_w = lr.w.detach().float().cpu().clone()
            out[pid] = (lr_w, lr.cum.detach().double().cpu().clone())
        return out
    finally:
        job.close()
