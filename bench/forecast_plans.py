"""Secondary bench: per-record forecast latency of scaled, polynomial, multi-class and
k-means pipelines — the one-row predict path (``--forecastServer true``, the baseline)
against the plan-driven resident wave (``--forecastServer plans``).

One job with file topics and four pipelines — SVM + StandardScaler, ORR +
PolynomialFeatures(2), MultiClassPA K = 4, K-means k = 16 — and, for a per-pipeline figure,
one job per pipeline alone; each in both modes. A record is appended to the forecasting
topic and timed until its Predictions are in the predictions topic, one record at a time
with the engine idle between ticks. Whether the native lane engaged is recorded.

The two modes are not timed alike end to end: the native lane stamps its own append, while
the Python lane is waited for from the bench thread with ``catch_up`` (20 µs sleeps, and the
GIL shared with the lane thread), which adds wake-up time to the baseline's p50 / p99. So
each result also carries ``lane_own_us``, the lane's own per-record latency (record polled →
Predictions produced, ``ForecastServer.latency_percentiles``) — the baseline figure to
compare against — and, for the Python lane, ``family_us`` per learner.

    python bench/forecast_plans.py [--records 1000] [--out profiles/round7/forecast_plans.json]

``--nonlinear``: the two learners ``plans`` leaves to one-row predicts — an NN with the
default hidden layers [32, 32] and an HT with the defaults, trained on the same block — are
added, and ``--forecastServer plans`` (the baseline here: those two are one-row predicts, the
code path of the commit before ``plans-all``) is compared with ``--forecastServer plans-all``
(both on the wave): the six pipelines in one job, and the NN and the HT each alone, whose
``publish_us`` is the cost of the two new ``serving_write``. Default output:
profiles/round7/forecast_plans_all.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from omldm_amd.api.batch import FeatureSpace  # noqa: E402

# 8 numerical + 8 categorical features: PolynomialFeatures(2) makes 44 dense lanes
NUM, CAT, DIM = 8, 8, 1 << 18
PIPELINES = {
    "SVM+StandardScaler": ("SVM", {}, ["StandardScaler"]),
    "ORR+PolynomialFeatures(2)": ("ORR", {}, ["PolynomialFeatures"]),
    "MultiClassPA(K=4)": ("MultiClassPA", {"nClasses": 4}, []),
    "K-means(k=16)": ("K-means", {"k": 16}, []),
}
NONLINEAR = {
    "NN[32,32]": ("NN", {}, []),
    "HT": ("HT", {}, []),
}


def _training_block(sp, n):
    """n training records, targets 0..3 by the first numerical feature."""
    from omldm_amd.io.synthetic import synth_json_records

    out = []
    for r in synth_json_records(n, sp):
        d = json.loads(r)
        x = d["numericalFeatures"][0]
        d["target"] = float(0 if x < -0.67 else 1 if x < 0 else 2 if x < 0.67 else 3)
        out.append(json.dumps(d))
    return ("\n".join(out) + "\n").encode()


def _pct(lat):
    lat = sorted(lat)
    if not lat:
        return {"p50": None, "p99": None, "n": 0}
    return {"p50": round(lat[len(lat) // 2], 2),
            "p99": round(lat[min(len(lat) - 1, int(0.99 * len(lat)))], 2), "n": len(lat)}


def measure(mode: str, names: list[str], n: int, block: bytes, recs: list[bytes]) -> dict:
    from omldm_amd.engine.job import Job
    from omldm_amd.io.transport import FileBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=shm) as root:
        br = FileBroker(root)
        for t in ("trainingData", "forecastingData", "requests", "predictions", "responses",
                  "performance"):
            br.create_topic(t, 1)
        args = []
        for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
                  "predictionsAddr", "performanceAddr"):
            args += [f"--{k}", f"file://{root}"]
        args += ["--numFeatures", str(NUM), "--catFeatures", str(CAT), "--hashDim", str(DIM),
                 "--batchSize", "8192", "--parallelism", "8", "--test", "false",
                 "--forecastServer", mode]
        job = Job(JobConfig.from_args(args), Comm.local(),
                  torch.device("cuda", torch.cuda.current_device()))
        try:
            for i, name in enumerate(names):
                learner, hyper, pre = {**PIPELINES, **NONLINEAR}[name]
                br.produce("requests", json.dumps({
                    "id": i + 1, "request": "Create",
                    "learner": {"name": learner, "hyperParameters": hyper},
                    "preProcessors": [{"name": p} for p in pre],
                    "trainingConfiguration": {"protocol": "Synchronous"}}))
            tfd = os.open(os.path.join(root, "trainingData", "0.jsonl"),
                          os.O_WRONLY | os.O_APPEND)
            os.write(tfd, block)
            os.close(tfd)
            for _ in range(3):
                job.tick()
            torch.cuda.current_stream().synchronize()
            fs = job.fserver
            # what a publish adds to a tick (each served writer's serving_write — for ORR
            # the fp64 Cholesky solve of weights() — on the training stream): host enqueue
            # and device time of one publish, medians of 20, each waited for by its event
            pub_host, pub_dev = [], []
            for _ in range(20):
                for _, pipe in sorted(job.pipes.items()):
                    if hasattr(pipe.learner, "_w"):
                        pipe.learner._w = None  # ORR: as after a round, weights() solves again
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                e0.record()
                fs.publish()
                e1.record()
                pub_host.append((time.perf_counter() - t) * 1e6)
                e1.synchronize()
                pub_dev.append(e0.elapsed_time(e1) * 1e3)
            ffd = os.open(os.path.join(root, "forecastingData", "0.jsonl"),
                          os.O_WRONLY | os.O_APPEND)

            def send(batch):
                lat = []
                for r in batch:
                    k = fs.native_stats()["served"] if fs.native else None
                    t_in = time.perf_counter()
                    os.write(ffd, r + b"\n")
                    if fs.native:
                        if not fs.native_wait(k + 1, 5.0):
                            raise RuntimeError("native forecast lane: no answer within 5 s")
                        t_out = fs.native_tout(k)
                    else:
                        if not fs.catch_up(5.0):
                            raise RuntimeError("forecast lane: no answer within 5 s")
                        t_out = time.perf_counter()
                    lat.append((t_out - t_in) * 1e6)
                    t = time.perf_counter()
                    while time.perf_counter() - t < 100e-6:  # records arrive one at a time
                        time.sleep(0)
                return lat

            send(recs[:20])  # wave start, warm caches
            lat = send(recs[20:20 + n])
            os.close(ffd)
            out = {"native_lane": bool(fs.native),
                   "on_wave": [names[pid - 1] for pid, _, _ in fs._served],
                   "one_row": [names[pid - 1] for pid, _ in fs._direct], **_pct(lat),
                   # the lane's own clock, record polled -> Predictions produced (warm-up
                   # records included): the figure free of the bench thread's waiting
                   "lane_own_us": fs.latency_percentiles(),
                   "publish_us": {"host_enqueue_p50": _pct(pub_host)["p50"],
                                  "device_p50": _pct(pub_dev)["p50"]}}
            trees = {names[pid - 1]: int(pipe.learner.nnodes.item())
                     for pid, pipe in sorted(job.pipes.items()) if pipe.learner.NAME == "HT"}
            if trees:
                out["tree_nodes"] = trees
            if fs.native:
                out["native_stage_us"] = fs.native_stats()["stage_us"]
            else:
                out["family_us"] = fs.family_percentiles()
            return out
        finally:
            job.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nonlinear", action="store_true",
                    help="add an NN and an HT; compare plans with plans-all")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "round7", "forecast_plans_all.json"
                             if a.nonlinear else "forecast_plans.json")
    from omldm_amd.io.synthetic import synth_json_records

    sp = FeatureSpace(NUM, 0, CAT, DIM)
    block = _training_block(sp, 20000)
    recs = [(r if isinstance(r, bytes) else r.encode()).replace(b"\n", b" ")
            for r in synth_json_records(a.records + 20, sp, start=10**9,
                                        operation="forecasting")]
    res = {"bench": "forecast_plans", "device": torch.cuda.get_device_name(0),
           "records": a.records, "space": {"numerical": NUM, "categorical": CAT, "dim": DIM},
           "unit": "us per record, appended to the forecasting topic -> Predictions appended",
           "baseline_flag": "true", "plans_flag": "plans", "job": {}, "alone": {}}
    names = list(PIPELINES)
    modes = (("true", "baseline"), ("plans", "plans"))
    alone = names
    if a.nonlinear:
        res["bench"] = "forecast_plans_all"
        res["baseline_flag"], res["plans_flag"] = "plans", "plans-all"
        names = names + list(NONLINEAR)
        modes = (("plans", "baseline"), ("plans-all", "plans"))
        alone = list(NONLINEAR)
    for mode, key in modes:
        res["job"][key] = measure(mode, names, a.records, block, recs)
        print(json.dumps({"job": key, **res["job"][key]}), flush=True)
    for name in alone:
        res["alone"][name] = {}
        for mode, key in modes:
            r = measure(mode, [name], a.records, block, recs)
            res["alone"][name][key] = r
            print(json.dumps({"alone": name, "mode": key, **r}), flush=True)
        b, p = res["alone"][name]["baseline"]["p50"], res["alone"][name]["plans"]["p50"]
        res["alone"][name]["plans_p50_below_baseline"] = bool(p < b)
        res["alone"][name]["plans_p50_below_baseline_lane_own"] = bool(
            p < res["alone"][name]["baseline"]["lane_own_us"]["p50"])
    b, p = res["job"]["baseline"]["p50"], res["job"]["plans"]["p50"]
    res["job"]["plans_p50_below_baseline"] = bool(p < b)
    res["job"]["plans_p50_below_baseline_lane_own"] = bool(
        p < res["job"]["baseline"]["lane_own_us"]["p50"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
