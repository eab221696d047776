#!/usr/bin/env python3
"""Do the frames in flight have a hardware queue each?  (DESIGN.md par. 7, "Frames in flight and hardware queues".)
Run on the GPU box.

  slot_queues.py                      the sweep: the pipelined step of the bench workload (1 M-point frames resident in HBM,
                                      cylinder RANSAC in the step) for 1..6 frames in flight under every value of
                                      GM_STREAM_PRIORITY, the values interleaved in child processes, three rounds, once in
                                      the environment as the box gives it and once with GPU_MAX_HW_QUEUES=8; per child also
                                      four frames in flight with a /choppedCloud output registered on every slot, and the
                                      blocking one-frame time of device-resident rows.  Medians over the rounds.
  slot_queues.py --ab <tagA> <tagB>   also `bench.py --gpus 1 --steps 200 --warmup 10` of two library builds
                                      (build/variants/libgm_hip_<tag>.so, tools/ab_refs.sh), alternated, three pairs, in both
                                      environments; the bench lines are kept whole
  slot_queues.py --queues DIR         from a `rocprofv3 --kernel-trace --output-format csv` run of the bench under DIR: the
                                      distinct queue ids of the k_normals<false> dispatches, and the dispatches on each
  slot_queues.py --traces NAME=DIR .. adds that, and tools/pipeline_overlap.py's figures of the same trace, to the file
                                      under kernel_traces.NAME (needs no GPU)
Writes profiles/r14_slot_queues.json (--out) unless --queues is given."""
import argparse, csv, glob, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = ("default", "high")
QVAR = "GPU_MAX_HW_QUEUES"


def queues(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    per, streams = {}, {}
    for r in csv.DictReader(open(f)):
        if "k_normals<false>" in r["Kernel_Name"]:
            per[r["Queue_Id"]] = per.get(r["Queue_Id"], 0) + 1
            if "Stream_Id" in r:
                streams.setdefault(r["Queue_Id"], set()).add(r["Stream_Id"])
    return {"k_normals_false_dispatches": sum(per.values()), "distinct_queue_ids": len(per), "dispatches_by_queue_id": per,
            "stream_ids_by_queue_id": {k: sorted(v) for k, v in streams.items()}}


def child(a):
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    import geometric_mapping_amd as g
    from geometric_mapping_amd import _lib, synth
    n = a.points
    r = synth.fixed_k_radius(n)
    dev = []
    for s in range(5):
        rows = np.zeros((n, 4), np.float32)
        rows[:, :3] = synth.tunnel_frame(n, seed=s)
        dev.append(torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    flags = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_CYLINDER
    kw = dict(neighborRadius=r, flags=flags, max_points=n, ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=1)

    def step_ms(c, clouds, slots, steps):
        def run(k):
            inflight = []
            for i in range(k):
                if len(inflight) == slots:
                    c.wait_frame(inflight.pop(0))
                c.submit_frame(i % slots, clouds[i % len(clouds)])
                inflight.append(i % slots)
            while inflight:
                c.wait_frame(inflight.pop(0))
        run(max(10, 3 * slots))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    out = {"GM_STREAM_PRIORITY": os.environ.get("GM_STREAM_PRIORITY"), QVAR: os.environ.get(QVAR)}
    with g.GeometricMapping(n_slots=a.max_slots, **kw) as c:
        clouds = [c.cloud_from_device(d.data_ptr(), n, 16) for d in dev]
        out["ms_per_step_by_frames_in_flight"] = {str(s): round(step_ms(c, clouds, s, a.steps), 4) for s in range(1, a.max_slots + 1)}
    with g.GeometricMapping(n_slots=4, **kw) as c:   # the node's default launch (displayCloud = true) on every slot
        clouds = [c.cloud_from_device(d.data_ptr(), n, 16) for d in dev]
        out["four_in_flight_ms_per_step"] = round(step_ms(c, clouds, 4, a.steps), 4)
        bufs = [c.cloud_output(s, n) for s in range(4)]
        out["four_in_flight_cloud_output_on_every_slot_ms_per_step"] = round(step_ms(c, clouds, 4, a.steps), 4)
        del bufs
    with g.GeometricMapping(n_slots=1, **kw) as c:
        clouds = [c.cloud_from_device(d.data_ptr(), n, 16) for d in dev]
        for i in range(5):
            c.process_frame(clouds[i % 5])
        ts = []
        for i in range(30):
            t0 = time.perf_counter()
            c.process_frame(clouds[i % 5])
            ts.append((time.perf_counter() - t0) * 1e3)
        out["blocking_frame_device_resident_rows_median_ms"] = round(float(np.median(ts)), 4)
    print(json.dumps(out))


def last_json(cmd, env, limit):
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(f"{' '.join(cmd)} ended with {p.returncode}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--queues", metavar="DIR")
    ap.add_argument("--ab", nargs=2, metavar="TAG")
    ap.add_argument("--traces", nargs="+", metavar="NAME=DIR")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--max-slots", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_slot_queues.json"))
    a = ap.parse_args()
    if a.queues:
        print(json.dumps(queues(a.queues), indent=1))
        return
    if a.traces:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_traces"] = {"command": "rocprofv3 --kernel-trace --output-format csv -- python bench.py --gpus 1 --steps 200 --warmup 10"}
        for item in a.traces:
            name, d = item.split("=", 1)
            ov = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pipeline_overlap.py"), d], capture_output=True, text=True, check=True)
            doc["kernel_traces"][name] = {"k_normals_queues": queues(d), "pipeline_overlap": json.loads(ov.stdout)}
            line = os.path.normpath(d) + ".json"   # (the bench line printed under the profiler, where the job kept it)
            if os.path.exists(line):
                with open(line) as f:
                    doc["kernel_traces"][name]["bench_line_under_profiler"] = json.loads(f.read().strip().splitlines()[-1])
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    if a.child:
        child(a)
        return
    doc = {"workload": f"{a.points}-point tunnel frames resident in HBM, fixed-k radius, cylinder RANSAC H = 1024, {a.steps} steps",
           "rounds": a.rounds, "environments": {}}
    for env_name, q in (("as_given", None), ("queues_8", "8")):
        env = dict(os.environ)
        if q:
            env[QVAR] = q
        runs = {v: [] for v in VALUES}
        for _ in range(a.rounds):
            for v in VALUES:
                runs[v].append(last_json([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps),
                                          "--points", str(a.points), "--max-slots", str(a.max_slots)],
                                         dict(env, GM_STREAM_PRIORITY=v), 300))
                print(env_name, v, json.dumps(runs[v][-1]), flush=True)
        row = {QVAR: env.get(QVAR), "by_GM_STREAM_PRIORITY": {}}
        for v in VALUES:
            by = {s: [r["ms_per_step_by_frames_in_flight"][s] for r in runs[v]] for s in runs[v][0]["ms_per_step_by_frames_in_flight"]}
            keys = ("four_in_flight_ms_per_step", "four_in_flight_cloud_output_on_every_slot_ms_per_step",
                    "blocking_frame_device_resident_rows_median_ms")
            row["by_GM_STREAM_PRIORITY"][v] = {
                "ms_per_step_by_frames_in_flight": {s: {"median": median(x), "runs": x} for s, x in by.items()},
                **{k: {"median": median([r[k] for r in runs[v]]), "runs": [r[k] for r in runs[v]]} for k in keys}}
        if a.ab:
            lines = {t: [] for t in a.ab}
            for _ in range(a.rounds):
                for t in a.ab:
                    lib = os.path.join(ROOT, "build", "variants", f"libgm_hip_{t}.so")
                    e = {k: v for k, v in env.items() if k != "GM_STREAM_PRIORITY"}
                    lines[t].append(last_json([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200",
                                               "--warmup", "10"], dict(e, GM_LIB_PATH=lib), 300))
                    print(env_name, t, json.dumps(lines[t][-1]), flush=True)
            ms = {t: [x["ms_per_step"] for x in lines[t]] for t in a.ab}
            row["bench_ab"] = {"command": "python bench.py --gpus 1 --steps 200 --warmup 10, alternated",
                               "ms_per_step": {t: {"median": median(ms[t]), "min": min(ms[t]), "max": max(ms[t]), "runs": ms[t]} for t in a.ab},
                               "bench_lines": lines}
        doc["environments"][env_name] = row
        with open(a.out, "w") as f:   # (after every environment: a later failure keeps what was measured)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
