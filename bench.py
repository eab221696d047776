#!/usr/bin/env python3
"""bench.py -- points/sec of the full per-frame path on MI355X (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path (ingest+crop -> cell sort -> radius normals ->
NaN compaction -> voxel grid -> scatter matrix + 3x3 eigen [-> RANSAC ext]) over one
synthetic 1M-point tunnel frame whose PointCloud2 rows are already resident in HBM.
Workload = BASELINE.json configs[1] ("1M-pt synthetic tunnel frame, single MI355X"),
fixed-k neighbour radius r = 0.5*sqrt(50000/N) (SURVEY.md par. 8d), launch-file values
for everything else.

N > 1 (one process per GPU, RCCL via torch.distributed):
  --mode frames (default): every rank runs its own stream of 1M-pt frames (frames are
      independent: BASELINE config 5); the only collective is one all-gather of the
      fitted records at the end of the timed region.  scaling = weak.
  --mode slab: ONE frame cut into x-slabs with a radius halo; per step each rank
      processes its slab, all-gathers a 10-double record (scatter partials + counts)
      over RCCL and solves the merged 3x3.  scaling = strong.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline keys
(metric, value, unit, ms_per_step, ... and config).  With --dump-outputs DIR it first writes the last timed step's
outputs (frame result, valid cloud with its input rows, normals, voxel centroids) as DIR/<name>.npy.
With --full the line also carries
  roofline          the dominant kernel's exclusive duration (frames one at a time, a run of its own) against HBM
  per_frame         SURVEY par. 8(d) / BASELINE.md par. 3 protocol: ONE blocking gm_process_frame per frame, rows handed
                    over as a HOST buffer (H2D inside), median / p10 / p90 of >= 20 frames after 3 warm-ups; pageable and
                    page-locked input, with and without the /choppedCloud D2H, and device-resident rows (kernels only)
  stress_launch_literal   the reference's own launch value neighborRadius = 0.5 on the same 1 M frame (k ~ 5 100)
  cpu_config1       BASELINE configs[0]: 50 k points, r = 0.5, oracle f32_faithful on 1 thread and on all usable cores
  (and cpu_baseline, whole_path_hbm and the other secondary rows: stage times, host input, lidar-shaped, sharded frame)
`value` itself stays the whole-job rate with the rows resident in HBM (the round contract: a PCIe-inclusive rate
is never `value`); `roofline.frac` uses the kernel's EXCLUSIVE duration (frames one at a time), the figure rocprofv3's
kernel stats show, and the PMC numbers are read from profiles/r<tag>_* of the newest round that holds them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md); measured copy peak 6290
HBM_MEASURED_GBS = 6290.0
ALGO_BYTES_PER_POINT = 40.0    # SURVEY.md par. 8d: 12 B/pt in + 28 B per cropped point out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--radius", type=float, default=None, help="default: fixed-k 0.5*sqrt(50000/points)")
    ap.add_argument("--mode", choices=("frames", "slab"), default="frames")
    ap.add_argument("--slots", type=int, default=4, help="frames in flight per GPU (HIP streams; 4 is the measured best once every "
                    "stream has a hardware queue of its own: GPU_MAX_HW_QUEUES below)")
    ap.add_argument("--fixed-slots", action="store_true", help="use --slots frames in flight as given (no calibration between slots - 1 and slots)")
    ap.add_argument("--ransac", type=int, default=1,
                    help="1: the step includes ONE RANSAC model (cylinder, H=1024: BASELINE configs[1]); 0: reference-faithful path only")
    ap.add_argument("--no-secondary", action="store_true", help="skip the extra reference-faithful / host-input legs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="nccl (= RCCL) is the real thing; gloo only rehearses the N>1 control flow on a 1-GPU box")
    ap.add_argument("--force-device", type=int, default=-1, help="rehearsal only: every rank uses this device")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--graph", type=int, default=0, help="1: the timed contexts replay their launch chains from captured hipGraphs (GM_CFG_GRAPH)")
    ap.add_argument("--distinct-frames", type=int, default=5, help="synthetic frames the stream cycles through (not a multiple of "
                    "--slots: a slot must not see the same frame every time)")
    ap.add_argument("--frames", type=int, default=24, help="frames of the per-frame (blocking, H2D-inclusive) protocol")
    ap.add_argument("--profile-tag", default=None, help="rNN prefix of the profiles/ files to quote (default: newest)")
    ap.add_argument("--group-points", type=int, default=10_000_000,
                    help="points of the sharded-frame row (gm_group, 4 ranks sharing this GPU: BASELINE configs[3] shape); 0: skip")
    ap.add_argument("--full", action="store_true",
                    help="also everything besides the headline: roofline (with its exclusive-kernel frames), the secondary rows "
                         "(--no-secondary) and the CPU baselines (--no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64)")
    return ap.parse_args()


def profile_path(name, tag=None):
    """profiles/<tag>_<name>; without a tag the newest round that holds the file."""
    import glob
    import re
    if tag:
        p = os.path.join(ROOT, "profiles", f"{tag}_{name}")
        return p if os.path.exists(p) else None
    best = None
    for p in glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{name}")):
        m = re.search(r"r(\d\d)_", os.path.basename(p))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), p)
    return best[1] if best else None


def quantiles(ms, n_points):
    a = np.asarray(ms, dtype=np.float64)
    med = float(np.median(a))
    return {"frames": int(a.size), "median_ms": med, "p10_ms": float(np.quantile(a, 0.1)), "p90_ms": float(np.quantile(a, 0.9)),
            "points_per_s": n_points / (med * 1e-3)}


def usable_cpus():
    """CPUs this process may really use: the affinity mask capped by the cgroup CPU quota (a GPU box shows all
    256 hardware threads but grants a 16-CPU quota per GPU; more threads than that only get throttled)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                      # cgroup v2: "<quota|max> <period>"
            q, per = f.read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:     # cgroup v1
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def cpu_baseline(points, radius, threads):
    """The oracle (f32-faithful restatement of the reference's PCL/Eigen path), timed on
    this box's host cores on ONE frame of the same workload.  Baseline only."""
    from geometric_mapping_amd import synth
    from oracle import oracle_c as oc
    oc.build()
    xyz = synth.tunnel_frame(points, seed=0)
    ncores = threads or usable_cpus()
    t0 = time.perf_counter()
    oc.process_frame(xyz, 5.0, radius, 0.5, 0.2, oc.F32_FAITHFUL, nthreads=ncores, want_outputs=False)
    dt_all = time.perf_counter() - t0
    # single thread = how the reference actually executes (ros::spin, non-OMP NormalEstimation).
    # Bounded sample: one fifth of the frame; density drops 5x, so r*sqrt(5) keeps k (~256) and
    # with it the work per point.
    sub = xyz[: points // 5]
    t0 = time.perf_counter()
    oc.process_frame(sub, 5.0, radius * np.sqrt(5.0), 0.5, 0.2, oc.F32_FAITHFUL, nthreads=1, want_outputs=False)
    dt_one = time.perf_counter() - t0
    return {"value": points / dt_all, "unit": "points/s", "cores": int(ncores), "kind": "port",
            "sample": f"1 frame of the same workload ({points} pts, r={radius:.4f}), oracle f32_faithful, OpenMP over query points",
            "single_thread_value": (points // 5) / dt_one,
            "single_thread_sample": f"{points // 5} pts at matched k (r*sqrt(5)), 1 thread"}


def cpu_config1(threads):
    """BASELINE configs[0]: the 50 k-point frame with the launch file's own values (r = 0.5), oracle f32_faithful on one
    thread (how the reference runs: ros::spin + non-OMP NormalEstimation) and on every usable core."""
    from geometric_mapping_amd import synth
    from oracle import oracle_c as oc
    oc.build()
    xyz = synth.tunnel_frame(50000, seed=0)
    out = {"points": 50000, "radius": 0.5, "kind": "port"}
    for name, nt in (("one_thread", 1), ("all_cores", threads or usable_cpus())):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            oc.process_frame(xyz, 5.0, 0.5, 0.5, 0.2, oc.F32_FAITHFUL, nthreads=nt, want_outputs=False)
            ts.append(time.perf_counter() - t0)
        out[name] = {"threads": int(nt), "median_ms": float(np.median(ts)) * 1e3, "points_per_s": 50000 / float(np.median(ts))}
    return out


DUMP_MAX_ROWS = 1 << 20   # per-point arrays take 36 B a row (44 with a sample's index): at most 46 MB of the 64 MB a dump
                          # may hold; a larger valid cloud is dumped as a fixed, seeded sample of this many rows


def dump_outputs(out_dir, c, slot, res, ransac_on):
    """What the timed path computed in its last step, as a caller of it receives it: the gm_wait_frame record and the
    slot's bulky outputs (valid cloud with its input rows, normals, voxel centroids), one float32 / float64 .npy each."""
    os.makedirs(out_dir, exist_ok=True)
    xyz, rows = c.cropped_cloud(slot)
    nrm = c.normals(slot)
    vox, vcount = c.voxel_centroids(slot)
    arrays = {"counts": np.array([res[k] for k in ("n_in", "n_cropped", "n_valid", "n_voxels")], dtype=np.float64),
              "status_flags": np.array([res["status_flags"]], dtype=np.float64),
              "eigenvalues": res["eigenvalues"], "eigenvectors": res["eigenvectors"], "center_axis": res["center_axis"],
              "scatter6": res["scatter6"], "voxel_centroids": vox, "voxel_counts": vcount.astype(np.float64)}
    if ransac_on:   # (the context fits the cylinder model only)
        arrays.update(cylinder=res["cylinder"], cylinder_inliers=np.array([res["cylinder_inliers"]], dtype=np.float64),
                      cylinder_axis_refit=res["cylinder_axis_refit"])
    if len(xyz) > DUMP_MAX_ROWS:
        pick = np.sort(np.random.default_rng(0).choice(len(xyz), DUMP_MAX_ROWS, replace=False))
        xyz, rows, nrm = xyz[pick], rows[pick], nrm[pick]
        arrays["sample_index"] = pick.astype(np.float64)
    arrays.update(valid_xyz=xyz, valid_input_rows=rows.astype(np.float64), normals=nrm)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype in (np.float32, np.float64) else a.astype(np.float64))


def roofline_rows(args, n, radius, mode, value, results, k_ms_excl):
    """--full: the dominant kernel against HBM (`roofline`) and the whole path's algorithmic bytes (`whole_path_hbm`)."""
    # dominant kernel: the neighbourhood-normals kernel, HIP-event bracketed on the stream it runs on
    # (gm_frame_result.normals_kernel_ms): in the timed region it shares the chip with the other frames in flight,
    # the roofline uses its exclusive duration (what rocprofv3's kernel stats of this command show)
    k_ms = float(np.mean([r["normals_kernel_ms"] for r in results])) if results else 0.0
    n_crop = float(np.mean([r["n_cropped"] for r in results])) if results else 0.0
    algo_bytes = 28.0 * n_crop                      # SURVEY par. 8d: normals = 12 N' read + 16 N' written
    k_roof = k_ms_excl if k_ms_excl else k_ms
    achieved = algo_bytes / (k_roof * 1e-3) / 1e9 if k_roof > 0 else 0.0
    traffic, traffic_src = None, None
    prof = profile_path("normals_pmc.json", args.profile_tag)
    if prof and mode == "frames":
        try:
            with open(prof) as f:
                pj = json.load(f)
            if pj.get("points") == n and abs(pj.get("radius", 0) - radius) < 1e-9:
                traffic, traffic_src = pj.get("hbm_bytes_per_launch"), os.path.relpath(prof, ROOT)
        except Exception:
            traffic = None
    # the kernel's real bound is instruction issue (VALU + MFMA), not HBM: busy fractions from the committed PMC pass
    # of the same workload; the live part is the instruction rate implied by that count and THIS run's duration
    valu = None
    vprof = profile_path("normals_valu_pmc.json", args.profile_tag)
    if vprof and mode == "frames":
        try:
            with open(vprof) as f:
                vj = json.load(f)
            insts = float(vj["counters"]["SQ_INSTS_VALU"])
            valu = {"valu_busy_frac_pmc": vj["derived"]["valu_busy_frac"], "SQ_INSTS_VALU_per_launch": insts,
                    "wave_instr_per_s": insts / (k_roof * 1e-3) if k_roof else None,
                    "peak_wave_instr_per_s_packed": 1024 * 2.4e9 / 4.0,
                    "mfma_busy_frac_pmc": vj["derived"].get("mfma_busy_frac"),
                    "source": os.path.relpath(vprof, ROOT)}
            # the matrix-core side of the same kernel: v_mfma_f32_32x32x16_bf16 = 2 * 32 * 32 * 16 flops per wave instruction
            mf = vj["counters"].get("SQ_INSTS_MFMA")
            if mf and k_roof:
                tf = float(mf) * 32768.0 / (k_roof * 1e-3) / 1e12
                valu["mfma"] = {"SQ_INSTS_MFMA_per_launch": float(mf), "achieved_TFLOPs_bf16": tf, "peak_TFLOPs_bf16_dense": 2500.0,
                                "frac": tf / 2500.0,
                                "note": "exact bf16 splits (3 terms per fp32 value) and 0/1 weights: flops of the formulation, "
                                        "not of an fp32 GEMM; the kernel is bound by the VALU work that feeds the products"}
        except Exception:
            valu = None
    return {
        "roofline": {"kernel": "k_normals",
                     "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                     "avg_launch_ms": k_roof, "avg_launch_ms_in_pipeline": k_ms,
                     "algorithmic_bytes_per_launch": algo_bytes, "issue": valu,
                     "note": "compute-bound neighbour loop (k~256; distances and moments on the matrix cores, near-threshold pairs re-evaluated exactly on the VALU): the HBM "
                             "fraction is reported as the contract asks, DESIGN.md par. 4 holds its issue-rate roofline. "
                             "avg_launch_ms = hipEvent bracket with frames one at a time (= rocprofv3 kernel stats of this "
                             "command); avg_launch_ms_in_pipeline = the same bracket inside the timed region, where the "
                             "kernel shares the chip with the other frames in flight"},
        "whole_path_hbm": {"algorithmic_bytes_per_point": ALGO_BYTES_PER_POINT,
                           "achieved_GBs": value * ALGO_BYTES_PER_POINT / 1e9,
                           "frac_of_spec": value * ALGO_BYTES_PER_POINT / 1e9 / HBM_PEAK_GBS},
    }


def main():
    args = parse()
    # ROCm multiplexes a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4): with the frames' streams
    # plus the runtime's own, a fourth frame in flight shares a queue with another and is serialised behind it (measured:
    # 4 slots 0.271 ms per step with 4 queues, 0.211 with 8; 3 slots 0.227 either way).  Read when the runtime initialises.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one process per GPU)")
        args.gpus = world

    import torch  # before libgm_hip: one HIP runtime per process (geometric_mapping_amd/_lib.py)
    import torch.distributed as dist

    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback to time)")
    if args.force_device >= 0:
        local_rank = args.force_device
    torch.cuda.set_device(local_rank)
    coll_dev = "cuda" if args.dist_backend == "nccl" else "cpu"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")

    import geometric_mapping_amd as g
    from geometric_mapping_amd import _lib, sharding, synth

    n = args.points
    radius = args.radius if args.radius else synth.fixed_k_radius(n)
    bound, leaf, wf = 5.0, 0.5, 0.2
    flags = _lib.GM_CFG_DEFAULT   # no per-stage events inside the timed region; a separate short run reads them
    if args.graph:
        flags |= _lib.GM_CFG_GRAPH
    ransac_on = False
    if args.ransac:
        probe = g.load_library()
        # the extension is part of the step only once its kernels exist in the library
        ransac_on = bool(getattr(probe, "gm_ext_available", None) and probe.gm_ext_available())
        if ransac_on:
            flags |= _lib.GM_CFG_RANSAC_CYLINDER

    def rows16(xyz):
        a = np.zeros((len(xyz), 4), dtype=np.float32)
        a[:, :3] = xyz
        return a

    n_slots = max(1, args.slots)
    mode = args.mode if world > 1 else "frames"
    if mode == "frames":
        n_frames = max(1, args.distinct_frames)
        frames_host = [synth.tunnel_frame(n, seed=1000 * rank + s) for s in range(n_frames)]
        dev = [torch.from_numpy(rows16(f)).cuda() for f in frames_host]
        pts_per_step_rank = n
        own = None
    else:
        full = synth.tunnel_frame(n, seed=0)
        edges = sharding.slab_edges(full, world, bound)
        rows = sharding.cut_slabs(full, edges, halo=radius * 1.01)[rank]
        dev = [torch.from_numpy(rows16(full[rows])).cuda()]
        pts_per_step_rank = None  # the frame is shared: n points per step for the whole job
        own = (edges[rank], edges[rank + 1])
        n_slots = 1
    torch.cuda.synchronize()

    tau_r = 0.03  # RANSAC inlier threshold (3 sigma of the generator), H = 1024 hypotheses per model

    def make_ctx(fl, slots):
        c = g.GeometricMapping(boxFilterBound=bound, voxelGridLeafSize=leaf, neighborRadius=radius, weightingFactor=wf,
                               device=local_rank, flags=fl, n_slots=slots, max_points=max(len(d) for d in dev),
                               ransac_hypotheses=1024, ransac_threshold=tau_r, ransac_seed=1 + rank)
        if own is not None:
            c.set_owned_range(*own)
        return c

    ctx = make_ctx(flags, n_slots)
    clouds = [ctx.cloud_from_device(d.data_ptr(), d.shape[0], 16) for d in dev]

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    rec_dev = torch.zeros(sharding.RECORD_LEN, dtype=torch.float64, device=coll_dev)
    gathered = torch.zeros(world * sharding.RECORD_LEN, dtype=torch.float64, device=coll_dev)

    prim_dev = torch.zeros(sharding.PRIMITIVE_LEN, dtype=torch.float64, device=coll_dev)
    prim_all = torch.zeros(world * sharding.PRIMITIVE_LEN, dtype=torch.float64, device=coll_dev)
    votes_dev = torch.zeros(2 * world, dtype=torch.int64, device=coll_dev)

    def slab_step(c):
        res = c.process_frame(clouds[0])
        rec_dev.copy_(torch.from_numpy(sharding.pack_record(res)))
        dist.all_gather_into_tensor(gathered, rec_dev)
        sc, _ = sharding.unpack_records(gathered.cpu().numpy())
        g.solve_local_frame(sharding.merge_scatter(sc))
        if ransac_on:
            # primitive vote (sharding.py): all-gather of every rank's fitted primitives, each rank counts every
            # candidate on its own resident slab, all-reduce of the counts, largest global count wins
            prim_dev.copy_(torch.from_numpy(sharding.pack_primitives(res)))
            dist.all_gather_into_tensor(prim_all, prim_dev)
            planes, cyls, _ = sharding.unpack_primitives(prim_all.cpu().numpy())
            v = np.zeros(2 * world, dtype=np.int64)
            ok = np.isfinite(cyls).all(axis=1)
            if ok.any():
                v[world:][ok] = c.score_frame(1, cyls[ok], tau_r)
            votes_dev.copy_(torch.from_numpy(v))
            dist.all_reduce(votes_dev, op=dist.ReduceOp.SUM)
            res["cylinder_voted"] = sharding.vote_primitives(cyls, votes_dev.cpu().numpy()[world:])
        return res

    def run(c, inputs, steps, slots, results):
        if mode == "slab":
            for i in range(steps):
                r = slab_step(c)
                if results is not None:
                    results.append(r)
            return
        # frames: keep `slots` frames in flight on their own HIP streams
        inflight = []
        for i in range(steps):
            slot = i % slots
            if len(inflight) == slots:
                r = c.wait_frame(inflight.pop(0))
                if results is not None:
                    results.append(r)
            c.submit_frame(slot, inputs[i % len(inputs)])
            inflight.append(slot)
        while inflight:
            r = c.wait_frame(inflight.pop(0))
            if results is not None:
                results.append(r)

    def timed(c, inputs, slots, min_warmup=0):
        res = []
        run(c, inputs, max(args.warmup, min_warmup), slots, None)
        barrier()
        t0 = time.perf_counter()
        run(c, inputs, args.steps, slots, res)
        if world > 1 and mode == "frames":
            # fitted records of every rank's last frame to every rank (the node publishes them all)
            rec_dev.copy_(torch.from_numpy(sharding.pack_record(res[-1])))
            dist.all_gather_into_tensor(gathered, rec_dev)
        barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt, res

    # Frames in flight: 3 or 4 of the context's slots, whichever steps faster on THIS box (the driver's round-3 run saw 3
    # beat 4 on the reference-faithful path, the builder's the opposite) -- a short calibration inside the warm-up, outside
    # the timed region; every rank takes the same decision (max over ranks of each candidate's time).
    calib = None
    if mode == "frames" and n_slots >= 4 and not args.fixed_slots:
        calib = {}
        run(ctx, clouds, max(args.warmup, 2 * n_slots), n_slots, None)
        for cand in (n_slots - 1, n_slots):
            barrier()
            t0 = time.perf_counter()
            run(ctx, clouds, 4 * n_slots, cand, None)
            barrier()
            tc = time.perf_counter() - t0
            if world > 1:
                tt = torch.tensor([tc], dtype=torch.float64, device=coll_dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                tc = float(tt.item())
            calib[cand] = tc / (4 * n_slots) * 1e3
        n_slots = min(calib, key=calib.get)
    dt, results = timed(ctx, clouds, n_slots)
    total_points = (n * args.steps * world) if mode == "frames" else (n * args.steps)
    value = total_points / dt
    if args.dump_outputs and rank == 0:
        # the last timed step ran on slot (steps - 1) % n_slots (run() above); nothing has run on that slot since
        dump_outputs(args.dump_outputs, ctx, (args.steps - 1) % n_slots, results[-1], ransac_on)

    secondary = {}
    k_ms_excl = None
    if args.full and mode == "frames":
        # the dominant kernel with the chip to itself: frames one at a time, hipEvents on the slot's own stream
        ex = [ctx.process_frame(clouds[i % len(clouds)])["normals_kernel_ms"] for i in range(max(10, min(args.steps, 30)))]
        k_ms_excl = float(np.mean(ex[2:]))
    if args.full and not args.no_secondary and world == 1:
        if ransac_on:  # the reference-faithful path alone (no extension work in the step)
            # (its shorter chain overlaps differently: measured with the step's number of slots and with one less)
            rows = {}
            for sl in sorted({n_slots, max(1, n_slots - 1)}):
                with make_ctx(_lib.GM_CFG_DEFAULT, sl) as c2:
                    dt2, _ = timed(c2, clouds, sl)
                rows[sl] = dt2
            best = min(rows, key=rows.get)
            secondary["reference_faithful_path_only"] = {"value": n * args.steps / rows[best], "ms_per_step": rows[best] / args.steps * 1e3,
                                                         "frames_in_flight": best,
                                                         "ms_per_step_by_frames_in_flight": {str(k): v / args.steps * 1e3 for k, v in rows.items()}}
        # per-stage device times of one frame alone (events on; outside every timed region)
        with make_ctx(flags | _lib.GM_CFG_STAGE_TIMING, 1) as c3:
            for _ in range(3):
                c3.process_frame(clouds[0])
            st = [c3.process_frame(clouds[i % len(clouds)])["stage_ms"] for i in range(8)]
            secondary["stage_ms_one_frame_alone"] = {k: round(float(np.median([x[k] for x in st])), 4) for k in st[0]}
        host_rows = [rows16(f) for f in frames_host]
        host_inputs = [ctx._cloud_from_xyz(r16) for r16 in host_rows]
        pinned_inputs = []
        for r16 in host_rows:
            buf, as_cloud = ctx.pinned_rows(r16.shape[0], 16)
            buf[:] = r16.reshape(-1).view(np.uint8)
            pinned_inputs.append(as_cloud())
        # ---- SURVEY par. 8(d) protocol: one blocking call per frame, median / p10 / p90
        import ctypes
        cloud_out = np.empty((n, 4), dtype=np.float32)      # the node's /choppedCloud message buffer, reused per frame
        cloud_ptr = cloud_out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        n_out = ctypes.c_uint32(0)

        def per_frame(inputs, fetch_cloud=False, c=None):
            c = c or ctx
            ms = []
            for i in range(3 + args.frames):
                t0 = time.perf_counter()
                c.process_frame(inputs[i % len(inputs)])
                if fetch_cloud:                               # gm_get_cropped_xyz straight into the reused buffer
                    st = c._L.gm_get_cropped_xyz(c._ctx, 0, cloud_ptr, n, ctypes.byref(n_out))
                    assert st == 0, st
                if i >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return quantiles(ms, n)
        # (a page-locked buffer's first DMA on a stream pays a one-time mapping cost: every (slot, buffer) pair is
        #  touched once before anything is timed -- with 20 timed steps that cost used to sit inside the timed region)
        for sl in range(n_slots):
            for pc in pinned_inputs + host_inputs:
                ctx.submit_frame(sl, pc)
                ctx.wait_frame(sl)
        secondary["per_frame"] = {
            "protocol": f"blocking gm_process_frame per frame, 3 warm-ups, {args.frames} timed frames, wall clock of the call",
            "host_rows_pageable": per_frame(host_inputs),
            "host_rows_pinned": per_frame(pinned_inputs),
            "host_rows_pinned_plus_choppedCloud_d2h": per_frame(pinned_inputs, fetch_cloud=True),
            "device_resident_rows": per_frame(clouds),
        }
        # the default launch (displayCloud = true): /choppedCloud into the caller's own page-locked message buffer while the
        # frame's tail still runs (gm_set_cloud_output), instead of a gm_get_cropped_xyz after it
        with make_ctx(flags, 1) as c5:
            msg_buf = np.zeros((n, 4), dtype=np.float32)
            c5.cloud_output_into(0, msg_buf)
            pin5 = []
            for r16 in host_rows:
                buf, as_cloud = c5.pinned_rows(r16.shape[0], 16)
                buf[:] = r16.reshape(-1).view(np.uint8)
                pin5.append(as_cloud())
            for pc in pin5:
                c5.process_frame(pc)
            secondary["per_frame"]["host_rows_pinned_plus_choppedCloud_overlapped"] = per_frame(pin5, c=c5)
            secondary["per_frame"]["host_rows_pageable_plus_choppedCloud_overlapped"] = per_frame(
                [c5._cloud_from_xyz(r16) for r16 in host_rows], c=c5)
        # the same with the launch chain replayed from a captured hipGraph (GM_CFG_GRAPH)
        gctx = make_ctx(flags | _lib.GM_CFG_GRAPH, 1)
        secondary["per_frame"]["device_resident_rows_graph_replay"] = per_frame(clouds, c=gctx)
        secondary["per_frame"]["host_rows_pinned_graph_replay"] = per_frame(pinned_inputs, c=gctx)
        gctx.close()
        # rows handed over as HOST buffers with frames in flight (never the headline value)
        dt3, _ = timed(ctx, host_inputs, n_slots, min_warmup=4 * n_slots)
        secondary["host_input_pcie_inclusive"] = {"value": n * args.steps / dt3, "ms_per_step": dt3 / args.steps * 1e3,
                                                  "input": "pageable host rows: staging copy on the calling thread + H2D"}
        dt4, _ = timed(ctx, pinned_inputs, n_slots, min_warmup=4 * n_slots)
        secondary["host_input_pinned_pcie_inclusive"] = {"value": n * args.steps / dt4, "ms_per_step": dt4 / args.steps * 1e3,
                                                         "input": "page-locked host rows (GM_CLOUD_PINNED): H2D only"}
        # ---- stress row: the reference's own launch value (launch/mapping.launch:9), k ~ 5 100 at 1 M points
        with g.GeometricMapping(boxFilterBound=bound, voxelGridLeafSize=leaf, neighborRadius=0.5, weightingFactor=wf,
                                device=local_rank, flags=_lib.GM_CFG_DEFAULT, n_slots=1, max_points=n) as c4:
            c4.process_frame(clouds[0])
            ms, km = [], []
            for i in range(5):
                t0 = time.perf_counter()
                r4 = c4.process_frame(clouds[i % len(clouds)])
                ms.append((time.perf_counter() - t0) * 1e3)
                km.append(r4["normals_kernel_ms"])
            secondary["stress_launch_literal"] = {"neighborRadius": 0.5, "k_regime": "launch-literal (~5 100 neighbours)",
                                                  "normals_kernel_ms": float(np.median(km)), "frame_ms": float(np.median(ms)),
                                                  "points_per_s": n / (float(np.median(ms)) * 1e-3), "input": "rows resident in HBM"}

        # ---- BASELINE configs[0] on the GPU: the 50 k-point frame with the launch file's own values (r = 0.5), one blocking
        # frame from pageable host rows with /choppedCloud on the host -- what mapping.launch does per callback
        x50 = synth.tunnel_frame(50000, seed=0)
        with g.GeometricMapping(boxFilterBound=bound, voxelGridLeafSize=leaf, neighborRadius=0.5, weightingFactor=wf,
                                device=local_rank, flags=_lib.GM_CFG_DEFAULT, n_slots=1, max_points=50000) as c6:
            buf6 = np.zeros((50000, 4), dtype=np.float32)
            c6.cloud_output_into(0, buf6)
            in6 = c6._cloud_from_xyz(rows16(x50))
            ms, km = [], []
            for i in range(3 + args.frames):
                t0 = time.perf_counter()
                r6 = c6.process_frame(in6)
                if i >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
                    km.append(r6["normals_kernel_ms"])
            secondary["gpu_config1"] = {"points": 50000, "radius": 0.5, "input": "pageable host rows, /choppedCloud delivered to a page-locked host buffer",
                                        **quantiles(ms, 50000), "normals_kernel_ms": float(np.median(km))}
        # ---- a lidar-shaped frame (synth.velodyne_tunnel: 64 rings x 1 800 azimuth steps, organised, NaN returns, 32-byte
        # XYZIR rows, density falling off with range), launch values: the blocking frame from pageable rows with the
        # /choppedCloud copy -- what the node does at 10 Hz (launch/mapping.launch:7-26)
        vmsg = synth.velodyne_tunnel(rings=64, az=1800, seed=7, point_step=32)
        vn = vmsg["height"] * vmsg["width"]
        with g.GeometricMapping(boxFilterBound=bound, voxelGridLeafSize=leaf, neighborRadius=0.5, weightingFactor=wf,
                                device=local_rank, flags=_lib.GM_CFG_DEFAULT, n_slots=1, max_points=vn) as c7:
            buf7 = np.zeros((vn, 4), dtype=np.float32)
            c7.cloud_output_into(0, buf7)
            in7 = c7.cloud_from_rows(vmsg["data"], vn, 32, vmsg["offsets"])
            ms, km = [], []
            for i in range(3 + args.frames):
                t0 = time.perf_counter()
                r7 = c7.process_frame(in7)
                if i >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
                    km.append(r7["normals_kernel_ms"])
            secondary["velodyne_like"] = {"points": vn, "rings": 64, "azimuth_steps": 1800, "point_step": 32, "radius": 0.5,
                                          "n_cropped": r7["n_cropped"], "n_valid": r7["n_valid"], "n_voxels": r7["n_voxels"],
                                          "input": "pageable host rows (NaN returns included), /choppedCloud delivered to a page-locked host buffer",
                                          **quantiles(ms, vn), "normals_kernel_ms": float(np.median(km))}

        # ---- one frame sharded over 4 ranks inside the C ABI (gm_group; the ranks share this GPU, so the records travel by
        # device copies and the four slabs' kernels queue on one device): where the time of gm_group_process_frame goes
        if args.group_points:
            gn = args.group_points
            gx = synth.tunnel_frame(gn, seed=3, floor_z=-1.2, outlier_frac=0.01)
            with g.GeometricMappingGroup([local_rank] * 4, loopback=True, boxFilterBound=bound, voxelGridLeafSize=leaf,
                                         neighborRadius=synth.fixed_k_radius(gn), weightingFactor=wf,
                                         flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER,
                                         ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=5) as gg:
                gg.process_frame(gx)
                ts = []
                for _ in range(3):
                    gg.process_frame(gx)
                    ts.append(gg.timing())
                edges, on_lattice = gg.edges()
            secondary["group_sharded_frame"] = {
                "points": gn, "ranks": 4, "transport": "loopback (4 ranks on one GPU; RCCL needs distinct devices)",
                "edges_on_voxel_lattice": on_lattice, "host_threads": min(16, usable_cpus()),
                **{k: round(float(np.median([t[k] for t in ts])), 3) for k in ts[0]},
                "note": "cut_ms = host: x histogram over the voxel lattice, edges, rows scattered into per-rank page-locked "
                        "buffers; device_ms = H2D + the four slabs' kernels one after the other on this one GPU + gather"}

    if rank == 0:
        out = {
            "metric": "points/sec full segment+fit, 1M-pt synthetic tunnel frame",
            "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak" if mode == "frames" else "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{n}-pt synthetic tunnel frame (R=2 m, L=12 m, sigma=0.01), rows resident in HBM",
                       "neighborRadius": radius, "k_regime": "fixed-k (~256 neighbours)", "boxFilterBound": bound,
                       "voxelGridLeafSize": leaf, "weightingFactor": wf, "mode": mode, "frames_in_flight": n_slots,
                       "frames_in_flight_calibration_ms_per_step": ({str(k): round(v, 4) for k, v in calib.items()} if calib else None),
                       "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                       "ransac_model": "cylinder, H=1024, tau=0.03 (extension)" if ransac_on else "none (reference-faithful path)",
                       "parallelism": f"{mode}x{world}", "collective_backend": args.dist_backend if world > 1 else None},
        }
        if args.full:
            out.update(roofline_rows(args, n, radius, mode, value, results, k_ms_excl))
            out.update(secondary)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(n, radius, args.cpu_threads)
                out["cpu_config1"] = cpu_config1(args.cpu_threads)
        print(json.dumps(out))
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
