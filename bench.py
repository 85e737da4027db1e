#!/usr/bin/env python3
"""bench.py -- typed reads/s of the hot path at HLA-A (BASELINE.json configs[1]) on N MI355X of one node.

A step = one pass of the hot path over one sample's read set that is already resident in HBM as the
front-end's piece batch: piece x allele compatibility -> per-pair class rows -> class dedup (gene and exon
level) -> Gene_counts -> EM #1 -> exon->gene hand-off -> EM #2 -> abundances.
N > 1: one process per GPU (torchrun), every rank types its own synthetic sample of the same locus (weak
scaling, no data-path collective); the shared locus index is broadcast once from rank 0 over RCCL.

Prints ONE JSON line on rank 0 (see DESIGN.md section 6 for the byte model behind `roofline`).  A plain run sets up, warms up,
times the steps and prints the line; `--full` adds everything else the benchmark measures or checks (the host front end's batch
against the device's, the file -> result legs, cpu_baseline, samples in flight, the bit-identical EM, the other workloads).
`--dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy (float64).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _launch_ranks_if_needed():
    """`python bench.py --gpus N` without a launcher: start N ranks (one per GPU) of this same script under
    torch.distributed.run as a CHILD process and exit with its code.  Runs before anything in this process has loaded
    libhgx or touched the GPU (a process that has initialised the GPU must not be replaced or forked into ranks).
    Under a launcher (WORLD_SIZE set) the world size must be the --gpus the caller asked for."""
    import subprocess
    n, backend, dry, share = 1, "nccl", False, False
    argv = sys.argv[1:]
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            n = int(argv[i + 1])
        elif a.startswith("--gpus="):
            n = int(a.split("=", 1)[1])
        elif a == "--backend" and i + 1 < len(argv):
            backend = argv[i + 1]
        elif a.startswith("--backend="):
            backend = a.split("=", 1)[1]
        elif a == "--dry-run":
            dry = True
        elif a == "--share-gpu":
            share = True
    if n < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != n:
            sys.exit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks" % (n, ws))
        return
    if n == 1:
        return
    if share and backend == "nccl" and not dry:
        sys.exit("bench.py: --share-gpu needs --backend gloo (RCCL refuses two ranks on one device)")
    if backend == "nccl" and not dry:
        import torch                      # device_count() does not initialise the GPU on this image
        have = torch.cuda.device_count()
        if have < n:
            sys.exit("bench.py: --gpus %d requested but this node has %d visible GPU(s); refusing to report n_gpus=1" % (n, have))
    import socket
    with socket.socket() as sk:           # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    sys.exit(subprocess.call(cmd, env=env))


if __name__ == "__main__":
    _launch_ranks_if_needed()

import numpy as np  # noqa: E402

import hisatgenotype_amd as hgx  # noqa: E402
from hisatgenotype_amd import capi, engine, synth  # noqa: E402
if os.environ.get("HGX_BENCH_LIB"):          # tools/bench_with_lib.py: an A/B against another build of libhgx (the child processes too)
    capi.LIB_PATH = os.environ["HGX_BENCH_LIB"]
htyping = sys.modules["hisatgenotype_amd.typing"]   # the module (the package also exports the typing() function)
from hisatgenotype_amd import locus as hl  # noqa: E402

N_TIMED_STEPS = 2         # steps (the last ones) whose EM mat-vec launches are all timed
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
LDS_READ_B32_PEAK_GBS = 75000.0   # aggregate ds_read_b32 rate with every CU streaming (MI355X_MICROARCH.md, LDS section)
PCIE_H2D_GBS = 57.5               # host -> device rate of registered host memory on the GPU box (tools/pinned_probe.hip)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=500000, help="read pairs per sample (1M reads = configs[1])")
    ap.add_argument("--alleles", type=int, default=7000)
    ap.add_argument("--vars", type=int, default=2500)
    ap.add_argument("--err", type=float, default=0.002)
    ap.add_argument("--cpu-pairs", type=int, default=20000, help="pairs of the same workload timed on the CPU oracle")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the file -> result measurements (SAM text and BAM; the N-process leg; the workloads' file legs)")
    ap.add_argument("--e2e-procs", default="1,2,4,8",
                    help="file -> result with N processes sharing GPU 0 (one sample stream each): the host-scaling leg of the --full run; '' skips it")
    ap.add_argument("--e2e-child", default=None, help=argparse.SUPPRESS)      # internal: one process of that leg (a JSON job description)
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the per-launch HIP events (profiling runs)")
    ap.add_argument("--workload", choices=["configs1", "class1", "panel64", "config0_dropin", "codis_dropin", "sample6"], default="configs1",
                    help="configs1 (default; BASELINE.json configs[1]: one HLA-A sample of 1 M reads per GPU), class1 (configs[2]: "
                         "HLA-A + B + C, 1 M reads each, loci -- and the reads of a locus -- sharded over the GPUs), panel64 "
                         "(configs[3]: six loci x 64 samples sharded over the GPUs)")
    ap.add_argument("--panel-pairs", type=int, default=5000, help="panel64: read pairs per (sample, locus) task")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl", help="torch.distributed backend (nccl = RCCL; gloo for --dry-run on CPU)")
    ap.add_argument("--dry-run", action="store_true",
                    help="rendezvous only: every rank joins the process group and rank 0 prints the world it saw (no GPU work)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="every rank on GPU 0 (with --backend gloo): the REAL multi-rank body -- sharding, exchanges, max-over-ranks timing -- "
                         "on a one-GPU box; the line says so (`shared_gpu`), its value is not a scaling figure")
    ap.add_argument("--comm", choices=["auto", "rccl", "torch"], default="auto",
                    help="exchanges of a sharded locus: auto = dist.RcclComm under nccl, dist.TorchComm under gloo; rccl = RcclComm whatever the "
                         "control plane (tests: HGX_BENCH_RCCL_LIB names a library with RCCL's entry points for ranks that share one GPU); torch = TorchComm")
    ap.add_argument("--check-unsharded", action="store_true",
                    help="class1: every rank of a sharded locus also types the whole locus alone and compares (`sharded_equals_unsharded`)")
    ap.add_argument("--no-in-flight", action="store_true", help="skip the side measurement with 2 / 3 samples in flight")
    ap.add_argument("--no-workloads", action="store_true", help="default workload only: skip the class1 / panel64 runs that follow it")
    ap.add_argument("--workloads", action="store_true", help="--full: run class1 / panel64 behind the default workload also with more than one rank "
                                                               "(by default they are N = 1 legs, like cpu_baseline and e2e: the scaling run is about `value`)")
    ap.add_argument("--wl-steps", type=int, default=10, help="timed steps of the class1 / panel64 runs that follow the default workload")
    ap.add_argument("--em-exact", action="store_true",
                    help="panel64: EM #1 in the reference's own order of floating-point operations (hgx_type_opts.em_fast = 0, the "
                         "library's default: bit-identical abundances) instead of the table-lookup arithmetic the throughput run uses; "
                         "configs1 / class1: em_fast = -1, the reference's order also for the > 4096-class exon-level EM (one CU: "
                         "the price of bit-identical abundances at that size)")
    ap.add_argument("--one-by-one", action="store_true", help="panel64: one launch chain per task (round 2's form) instead of hgx_type_many")
    ap.add_argument("--inflight", type=int, default=1,
                    help="samples typed concurrently per GPU (host threads with their own streams and class-row buffers; "
                         "the EM of one sample is a chain of short launches that leaves the GPU to the scoring of the next)")
    ap.add_argument("--full", action="store_true",
                    help="configs1: also run what the headline does not need -- the host front end's check of the device batch, the "
                         "file -> result legs (incl. --e2e-procs), cpu_baseline, samples in flight, the bit-identical EM and the other "
                         "workloads (the --no-* options above switch single legs off again)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="configs1: write what the last timed step returned (counts, both EMs, gene_prob) as DIR/<name>.npy in float64")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.workload != "configs1":
        ap.error("--dump-outputs covers the default workload (configs1) only")
    return args


COMM_FORCE = "auto"      # --comm: which exchange object the ranks of a sharded locus get (make_comm)
DIST_DEV = "cuda"        # device of the control-plane tensors (torch.distributed): "cuda" with nccl (= RCCL), "cpu" with gloo
EM_MODE = False          # --em-exact: -1 = the reference's order of operations at every size (hgx_type_opts.em_fast = -1)


def step(pl, batch, db, ev=None, stream=None, gate=None):
    """One pass of the hot path on `stream` (None = the default stream): ONE call into libhgx (hgx_type_dbatch) over the
    piece batch resident in HBM (`db`; the host `batch` may be None).  `ev` = (compat begin, compat end, pairs begin, pairs end)
    events.  Returns the LocusResult."""
    res = htyping.LocusResult()
    res.num_reads, res.num_pairs = db.n_reads, db.n_pairs
    return htyping._type_batch(pl, batch, res, True, dbatch=db, stream=stream, overlap=True, gate=gate, events=ev, em_fast=EM_MODE)


def run_steps(pl, batch, db, inflight, n_steps, ev_list, timing, local_rank):
    """n_steps passes shared by `inflight` host threads (one sample in flight per thread).  Returns
    (last LocusResult, EM seconds summed, EM iterations summed, merged per-kernel timing)."""
    import threading
    lock = threading.Lock()
    gate = engine.Gate() if inflight > 1 else None      # staggers the samples in flight (hgx_type_opts.gate)
    state = {"next": 0, "t_em": 0.0, "n_iter": 0, "res": None, "timing": {}, "err": None}

    def work(own_stream, slot=None):
        try:
            capi.set_device(local_rank)
            if slot is not None:
                capi.set_stream_slot(slot)           # the warm-up generation of this worker created the streams
            stream = capi.get_stream(2) if own_stream else None
            engine.em_set_timing(0)
            while True:
                with lock:
                    k = state["next"]
                    if k >= n_steps:
                        break
                    state["next"] = k + 1
                # every EM mat-vec launch of the LAST steps of the timed region is timed (dispatch-attached events); earlier
                # steps run untimed, so the ~1 us per timed launch does not weigh on the whole region
                engine.em_set_timing(2 if (timing and k >= n_steps - N_TIMED_STEPS) else 0)
                res = step(pl, batch, db, ev_list[k] if ev_list else None, stream, gate)
                with lock:
                    state["t_em"] += res.t_em
                    state["n_iter"] += sum(e["n_iter"] for e in res.em)
                    state["res"] = res
            capi.sync(stream)
            if timing:
                with lock:
                    for name, v in engine.em_get_timing().items():
                        acc = state["timing"].setdefault(name, [0.0, 0, 0, 0])
                        for i in range(4):
                            acc[i] += v[i]
        except BaseException as e:     # re-raised on the main thread
            state["err"] = e

    if inflight <= 1:
        work(False)
    else:
        threads = [threading.Thread(target=work, args=(True, i)) for i in range(inflight)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if state["err"] is not None:
        raise state["err"]
    return state["res"], state["t_em"], state["n_iter"], state["timing"]


def dump_outputs(out_dir, res, pl):
    """--dump-outputs: the LocusResult of the last timed step as float64 arrays, allele names as indices into pl.names (a few
    hundred KB at configs[1])."""
    os.makedirs(out_dir, exist_ok=True)
    aidx = {n: i for i, n in enumerate(pl.names)}
    arrs = {"reads_pairs": [res.num_reads, res.num_pairs],
            "counts": res.counts,                                  # Gene_counts per allele index
            "counts_order": res.counts_order,                      # allele indices in the reference's print order
            "gene_prob_allele": [aidx[a] for a, _ in res.gene_prob], "gene_prob": [p for _, p in res.gene_prob]}
    for k, em in enumerate(res.em):
        arrs["em%d_stats" % k] = [em["n_classes"], em["n_iter"], em["remove_low"], em["use_length"]]
        arrs["em%d_allele" % k] = [aidx[a] for a, _ in em["result"]]
        arrs["em%d_abundance" % k] = [p for _, p in em["result"]]
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float64))


def cpu_baseline(loc, sam, n_pairs):
    """The C oracle (1 core) on the first n_pairs pairs of the same workload: scoring + dedup + EM."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orclib
    import orc_pipeline
    import pyref
    import tables
    orc = orclib.load()
    lines = sam.split("\n", 2 * n_pairs)[:2 * n_pairs]
    sub = "\n".join(lines) + "\n"
    rl = pyref.RefLocus(loc)
    rl.score = False                      # front-end only: the haplotypes of each pair
    t0 = time.perf_counter()
    fe = rl.run(sub)
    t_front = time.perf_counter() - t0
    t = tables.oracle_tables(loc)
    arrs = tables.pieces_from_pairs(fe["pairs"], t["var_index"])
    lengths = np.array([loc.allele_length(n) for n in t["names"]], dtype=np.int32)
    out = orc_pipeline.run(orc, t, arrs, loc.base_fname == "hla", lengths)
    secs = out["t_score"] + out["t_dedup"] + out["t_em"]
    # pure-Python restatement (closest to the reference's own speed) on a much smaller slice
    n_py = min(150, n_pairs)
    rl2 = pyref.RefLocus(loc)
    t0 = time.perf_counter()
    r2 = rl2.run("\n".join(lines[:2 * n_py]) + "\n")
    t_py = time.perf_counter() - t0
    recorded = None
    try:                                   # the REAL reference's wall time on configs[0], recorded in the build container with its outputs
        import gzip
        with gzip.open(os.path.join(ROOT, "tests", "golden", "hla_7000_10k.json.gz"), "rb") as f:
            rt = json.loads(f.read().decode())["reference_timing"]
        recorded = {"reads_per_s": rt["records_per_s"], "seconds": rt["seconds"], "records": rt["sam_records"], "cpu": rt["cpu"],
                    "cores": rt["cores_used"], "where": "build container, not this box (the reference is Python and cannot travel); "
                                                        "first 5 000 pairs of this bench's read set; BASELINE.md section 4"}
    except Exception:
        pass
    return {
        "value": round(fe["num_reads"] / secs, 1), "unit": "reads/s", "cores": 1, "kind": "port",
        "reference_recorded": recorded,
        "sample": "first %d pairs (%d reads) of the same synthetic HLA-A read set; C oracle scoring %.2fs + dedup %.2fs + EM %.2fs "
                  "(%d outer iterations); front-end excluded on both sides" % (
                      n_pairs, fe["num_reads"], out["t_score"], out["t_dedup"], out["t_em"], out["n_iter"]),
        "em_iters_per_s": round(out["n_iter"] / max(out["t_em"], 1e-9), 2),
        "python_port_reads_per_s": round(r2["num_reads"] / t_py, 1),
        "python_port_sample": "oracle/pyref.py end to end (front-end included) on the first %d pairs" % n_py,
    }, out


def cpu_baseline_tasks(tasks, what):
    """The C oracle (1 core) on a bounded sample of a multi-task workload: `tasks` = [(synth locus, SAM text)]; scoring + dedup
    + EM summed over the tasks (front-end excluded on both sides, as in the headline's baseline)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orclib
    import orc_pipeline
    import pyref
    import tables
    orc = orclib.load()
    reads, secs, iters, t_em, t_sc = 0, 0.0, 0, 0.0, 0.0
    for loc, sam in tasks:
        rl = pyref.RefLocus(loc)
        rl.score = False
        fe = rl.run(sam)
        t = tables.oracle_tables(loc)
        arrs = tables.pieces_from_pairs(fe["pairs"], t["var_index"])
        lengths = np.array([loc.allele_length(n) for n in t["names"]], dtype=np.int32)
        out = orc_pipeline.run(orc, t, arrs, loc.base_fname == "hla", lengths)
        reads += fe["num_reads"]
        secs += out["t_score"] + out["t_dedup"] + out["t_em"]
        iters += out["n_iter"]
        t_em += out["t_em"]
        t_sc += out["t_score"] + out["t_dedup"]
    return {"value": round(reads / max(secs, 1e-9), 1), "unit": "reads/s", "cores": 1, "kind": "port",
            # the EM's cost is per TASK, the scoring's per READ: the sample's tasks are smaller than the GPU line's (disclosed in
            # `sample`), so the two parts are given separately -- a like-for-like CPU time for the GPU line's task size is
            # reads / scoring_dedup_reads_per_s + tasks x em_seconds_per_task
            "split": {"scoring_dedup_reads_per_s": round(reads / max(t_sc, 1e-9), 1), "em_seconds_per_task": round(t_em / max(len(tasks), 1), 4),
                      "tasks": len(tasks)},
            "sample": "%s: %d reads, C oracle scoring + dedup + EM %.2f s (%d outer EM iterations); front-end excluded on both sides" % (
                what, reads, secs, iters),
            "em_iters_per_s": round(iters / max(t_em, 1e-9), 2)}


def em_roofline(em_timing, n_timed_steps):
    """roofline object of a workload whose EM passes were timed with dispatch-attached events (engine.em_set_timing(2))."""
    kernels = {}
    for name, (ms, n, ex, by) in em_timing.items():
        if n:
            kernels[name] = {"timed_launches": n, "timed_steps": n_timed_steps, "alg_bytes_per_launch": int(by // n), "avg_ms": round(ms / n, 5),
                             "total_ms_per_step": round(ms / n_timed_steps, 4), "GBps": round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else 0.0}
    if not kernels:
        return None
    dom = max(kernels, key=lambda k: kernels[k]["total_ms_per_step"])
    k = kernels[dom]
    return {"bound": "hbm", "kernel": dom, "achieved": k["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(k["GBps"] / HBM_PEAK_GBS, 4),
            "traffic": None, "alg_bytes_per_launch": k["alg_bytes_per_launch"], "avg_launch_ms": k["avg_ms"],
            "note": "EM mat-vec pass with the largest aggregate time per step (every plain rows / cols pass of the last %d steps timed with "
                    "dispatch-attached HIP events); algorithmic bytes per pass = the compact class bit matrix once + its dense vectors" % n_timed_steps,
            "kernels": kernels}


def cgroup_cpu_quota():
    """CPUs' worth of CPU time per period this container may use (cgroup v2 cpu.max / v1 cfs quota), or None."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return q / per if q > 0 and per > 0 else None
    except Exception:
        return None


def cgroup_throttled_usec():
    """Total time this container's threads were frozen by the CPU-bandwidth controller (cgroup v2 cpu.stat), or None."""
    try:
        for line in open("/sys/fs/cgroup/cpu.stat"):
            if line.startswith("throttled_usec"):
                return int(line.split()[1])
    except Exception:
        pass
    return None


def end_to_end(pl, loc, sam, ref_res, runs=5):
    """File -> typing result through ONE C call (hgx_type_file): read (pread / BGZF inflate / BAM decode / name grouping),
    front-end, upload, GPU path, result on the host.  SAM text as an aligner writes it (grouped by read) and BAM as the
    reference's pipeline stores it (`samtools sort`: by coordinate), both from the page cache.  Two regimes after one warm-up
    call: `runs` calls 0.3 s apart (one sample at a time: the call's own latency -- `reads_per_s` / `ms`, the median) and `runs`
    calls back to back (`back_to_back`: a sample stream; the host side is CPU-TIME bound there and a container's CPU quota
    throttles it -- `throttled_ms` is the time the cgroup reports the process frozen during those calls)."""
    import ctypes as C
    import resource
    import tempfile
    from hisatgenotype_amd import bamio
    d = tempfile.mkdtemp(prefix="hgx_e2e_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {}
    L = capi.lib()
    try:
        paths = {"sam": os.path.join(d, "reads.sam"), "bam": os.path.join(d, "reads.bam")}
        data = sam.encode()
        with open(paths["sam"], "wb") as f:
            f.write(data)
        bamio.write_bam_native(paths["bam"], data, [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
        n_records = data.count(b"\n")
        del data
        def one_call(path, want_result):
            o = capi.ParseOpts(2, 1, 0, 0, 0, 0, 0, 0)
            to = htyping.TypeOpts(1, 0, -1, 0, None, None, None, None, None)
            h = C.c_void_p()
            t0 = time.perf_counter()
            capi.check(L.hgx_type_file(C.byref(h), pl.h, pl.index(), path.encode(), pl.ref_allele.encode(), C.byref(o), C.byref(to), None))
            dt = time.perf_counter() - t0
            res = None
            try:
                if want_result:
                    res = htyping.LocusResult()
                    nr, npair = C.c_int32(), C.c_int32()
                    capi.check(L.hgx_typing_dims(h, C.byref(nr), C.byref(npair), None, None, None, None, None, None))
                    res.num_reads, res.num_pairs = nr.value, npair.value
                    htyping._result_from_handle(h, pl, res, False)
            finally:
                L.hgx_typing_destroy(h)
            return dt, res

        for kind, path in paths.items():
            one_call(path, False)                                   # warm-up (pool blocks, page cache, streams)
            time.sleep(0.3)
            th0, ru0 = cgroup_throttled_usec(), resource.getrusage(resource.RUSAGE_SELF)
            times, res = [], None
            for rep in range(runs):
                dt, r = one_call(path, rep == runs - 1)
                res = r or res
                times.append(dt)
            th1, ru1 = cgroup_throttled_usec(), resource.getrusage(resource.RUSAGE_SELF)
            spaced = []
            for rep in range(runs):
                time.sleep(0.3)
                spaced.append(one_call(path, False)[0])
            th2 = cgroup_throttled_usec()
            same = (res.num_reads == ref_res.num_reads and res.gene_prob == ref_res.gene_prob and
                    [e["n_iter"] for e in res.em] == [e["n_iter"] for e in ref_res.em])
            med = sorted(times)[len(times) // 2]
            med_s = sorted(spaced)[len(spaced) // 2]
            cpu_s = (ru1.ru_utime + ru1.ru_stime - ru0.ru_utime - ru0.ru_stime) / runs
            route, code = engine.front_last()
            sent = engine.front_last_bytes()
            out[kind] = {"reads_per_s": round(res.num_reads / med_s, 1), "ms": round(med_s * 1e3, 2), "best_ms": round(min(spaced) * 1e3, 2),
                         "front_end": {"route": {2: "record route: " + ("BGZF inflate, record walk, region filter, name sort, " if kind == "bam" else "") +
                                                    "fields, filters, key grouping, pileup, decode, piece table, pair protocol as kernels",
                                                 1: "key route: host tokenises / filters / groups, the rest as kernels",
                                                 0: "host stages"}[route], "decline_code": code, "bytes_to_device": sent,
                                       "text_in_parts": engine.front_last_parts()},      # 3 = six eighths' lines + fields beside the seventh's transfer, the seventh's beside the eighth's
                         "roofline": {"bound": "pcie", "achieved": round(sent / med_s / 1e9, 2), "peak": PCIE_H2D_GBS, "unit": "GB/s",
                                      "frac": round(sent / med_s / 1e9 / PCIE_H2D_GBS, 4),
                                      "note": ("bytes the call sends to the device (the SAM text + its line table) / the call's time, against the measured "
                                               "host-to-device rate of registered memory (tools/pinned_probe.hip: 57.5 GB/s; PCIe Gen5 x16)") if kind == "sam" else
                                              ("a BAM travels DEFLATED (the file's bytes + a block table): the link is idle; the call is bound by "
                                               "k_bgzf_inflate_w -- DEFLATE symbol decoding, one wavefront per BGZF block, ~140 GB/s of payload -- and "
                                               "the record kernels behind it (DESIGN.md section 5.6)")},
                         "runs_ms": [round(t * 1e3, 1) for t in spaced],
                         "throttled_ms": None if th1 is None else round((th2 - th1) / 1e3, 1),
                         "cpu_seconds_per_call": round(cpu_s, 3),
                         "back_to_back": {"reads_per_s": round(res.num_reads / med, 1), "ms": round(med * 1e3, 2),
                                          "runs_ms": [round(t * 1e3, 1) for t in times],
                                          "throttled_ms": None if th0 is None else round((th1 - th0) / 1e3, 1)},
                         "file_MB": round(os.path.getsize(path) / 1e6, 1),
                         "records_in_file": n_records, "result_identical_to_hbm_path": bool(same)}
            try:            # dispatches / kernel time per call, from the committed kernel stats of the traced calls (tools/install_profiles_r05.py)
                prof = json.load(open(os.path.join(ROOT, "profiles", "step_profile.json"))).get("file_to_result", {}).get(kind)
                if prof and n_records == 1000000:
                    out[kind]["profile"] = prof
            except Exception:
                pass
            if kind == "bam":
                # the like-for-like CPU figure of a file -> result call: the HOST front end (csrc/hgx_sam.cpp + hgx_bam.cpp: read, inflate,
                # walk, sort, decode -- what the device front end is checked against) on ONE thread over the same file; the scoring +
                # EM part is the C oracle's (cpu_baseline: a bounded sample, its rate is applied to this file's reads by the caller)
                t0 = time.perf_counter()
                hb = pl.parse_alignment_file(path, regions=[pl.ref_allele], n_threads=1)
                out[kind]["host_front_end_one_thread_s"] = round(time.perf_counter() - t0, 3)
                del hb
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    quota = cgroup_cpu_quota()
    out["host"] = {"hw_threads": os.cpu_count(), "cgroup_cpu_quota": quota,
                   "front_end_threads": "2 x quota" if quota else "all hardware threads"}
    out["note"] = ("hgx_type_file per call: file (page cache) -> typing result on the host, H2D and the GPU path included; "
                   "reads_per_s / ms = median of %d calls 0.3 s apart after a warm-up (the call's own latency); back_to_back = the "
                   "same calls without a pause (a sample stream: bound by the CPU seconds the container's cgroup grants -- %s CPUs, "
                   "whatever the number of hardware threads; throttled_ms = time the cgroup froze the process during those calls)."
                   % (runs, "%.0f" % quota if quota else "all"))
    return out


# ---- file -> result with N processes sharing one GPU: how far does the HOST side scale? ----------------------------------------
# The reference's unit of scale is one process per sample (/root/reference/hisatgenotype:613-665).  N fresh child processes, started
# BEFORE this process touches the GPU, each type their own copy of the sample file K times back to back against GPU 0 after a
# warm-up call; they start together (a "go" file) and report their call times, CPU seconds and end time.  samples/s = N * K / (last
# end - go).
def _e2e_child(job_json):
    import ctypes as C
    import resource
    job = json.loads(job_json)
    pl = hl.PackedLocus.load_cache(job["cache"])
    capi.set_device(0)
    pl.index()
    L = capi.lib()

    def one_call():
        o = capi.ParseOpts(2, 1, 0, 0, 0, 0, 0, 0)
        to = htyping.TypeOpts(1, 0, -1, 0, None, None, None, None, None)
        h = C.c_void_p()
        t0 = time.perf_counter()
        capi.check(L.hgx_type_file(C.byref(h), pl.h, pl.index(), job["path"].encode(), pl.ref_allele.encode(), C.byref(o), C.byref(to), None))
        dt = time.perf_counter() - t0
        nr = C.c_int32()
        capi.check(L.hgx_typing_dims(h, C.byref(nr), None, None, None, None, None, None, None))
        L.hgx_typing_destroy(h)
        return dt, nr.value
    one_call()
    one_call()
    open(os.path.join(job["sync"], "ready_%d" % job["idx"]), "w").close()
    go = os.path.join(job["sync"], "go")
    while not os.path.exists(go):
        time.sleep(0.0005)
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    times, reads = [], 0
    for _ in range(job["calls"]):
        dt, nr = one_call()
        times.append(dt)
        reads += nr
    end = time.time()
    ru1 = resource.getrusage(resource.RUSAGE_SELF)
    route, code = engine.front_last()
    print(json.dumps({"idx": job["idx"], "times": times, "reads": reads, "end": end, "route": route, "decline_code": code,
                      "cpu_s": ru1.ru_utime + ru1.ru_stime - ru0.ru_utime - ru0.ru_stime}))


def e2e_scaling(loc, sam, procs, calls=6):
    """The host-scaling leg (parent side; no GPU call in this process yet).  Returns the `e2e_scaling` object of the JSON line."""
    import shutil
    import tempfile
    from hisatgenotype_amd import bamio
    d = tempfile.mkdtemp(prefix="hgx_e2e_procs_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"calls_per_process": calls, "host": {"hw_threads": os.cpu_count(), "cgroup_cpu_quota": cgroup_cpu_quota()}, "bam": {}, "sam": {}}
    try:
        pl = hl.PackedLocus.from_synth(loc)                     # (host tables only: no device index is made here)
        cache = os.path.join(d, "locus.npz")
        pl.save_cache(cache)
        data = sam.encode()
        n_records = data.count(b"\n")
        paths = {"sam": os.path.join(d, "reads.sam"), "bam": os.path.join(d, "reads.bam")}
        with open(paths["sam"], "wb") as f:
            f.write(data)
        bamio.write_bam_native(paths["bam"], data, [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
        del data
        for kind in ("bam", "sam"):
            for n in procs:
                sync = tempfile.mkdtemp(prefix="sync_", dir=d)
                files = []
                for i in range(n):                              # every process its own file (BAM: a copy; SAM text: one 400 MB file, shared)
                    if kind == "bam":
                        fp = os.path.join(sync, "reads_%d.bam" % i)
                        shutil.copyfile(paths["bam"], fp)
                    else:
                        fp = paths["sam"]
                    files.append(fp)
                kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--e2e-child",
                                          json.dumps({"cache": cache, "path": files[i], "sync": sync, "idx": i, "calls": calls})],
                                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(n)]
                t_wait = time.time()
                while sum(os.path.exists(os.path.join(sync, "ready_%d" % i)) for i in range(n)) < n:
                    if any(k.poll() is not None for k in kids) or time.time() - t_wait > 300:
                        break
                    time.sleep(0.005)
                th0 = cgroup_throttled_usec()
                go = time.time()
                open(os.path.join(sync, "go"), "w").close()
                res = []
                for k in kids:
                    so, se = k.communicate(timeout=600)
                    if k.returncode != 0:
                        raise RuntimeError("e2e child failed: " + se[-2000:])
                    res.append(json.loads(so.strip().splitlines()[-1]))
                th1 = cgroup_throttled_usec()
                wall = max(r["end"] for r in res) - go
                all_t = sorted(t for r in res for t in r["times"])
                out[kind][str(n)] = {"processes": n, "calls": n * calls, "wall_s": round(wall, 4),
                                     "samples_per_s": round(n * calls / wall, 2), "reads_per_s": round(sum(r["reads"] for r in res) / wall, 1),
                                     "ms_per_call_median": round(all_t[len(all_t) // 2] * 1e3, 2),
                                     "cpu_seconds_per_call": round(sum(r["cpu_s"] for r in res) / (n * calls), 3),
                                     "throttled_ms": None if th0 is None else round((th1 - th0) / 1e3, 1),
                                     "front_end_route": sorted(set(r["route"] for r in res))}
                shutil.rmtree(sync, ignore_errors=True)
        out["records_per_sample"] = n_records
        out["note"] = ("N processes (started before the parent touched the GPU), each typing its own copy of the sample file %d times back to back "
                       "through hgx_type_file against GPU 0 after two warm-up calls; samples_per_s = N x %d / (last end - common start).  The GPU "
                       "work of a call is ~7 ms (device front end + typing): beyond that the sample rate is bound by the CPU seconds the "
                       "container's cgroup grants (cpu_seconds_per_call x samples_per_s vs the quota)." % (calls, calls))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


CLASS1 = [("A", 7000, 3569, 2500, 101), ("B", 8000, 4081, 2800, 102), ("C", 7000, 4305, 2600, 103)]
PANEL = [("A", 7000, 3569, 2500), ("B", 8000, 4081, 2800), ("C", 7000, 4305, 2600), ("DRB1", 3000, 3800, 1800),
         ("DQA1", 500, 3300, 600), ("DQB1", 2000, 3600, 1400)]


def _torch_sync():
    """torch's own streams (the nccl collectives of the control plane run there); nothing to wait for with gloo."""
    if DIST_DEV == "cuda":
        import torch
        torch.cuda.synchronize()


def make_comm(dist, group=None):
    """The exchanges of a sharded locus for the ranks of `group`: with nccl this library's own RCCL communicator (dist.RcclComm:
    hgx_classes_allgather / hgx_allreduce_sum_* on device buffers, nothing through the host per step); with gloo (CPU control plane;
    --share-gpu) dist.TorchComm.  If the RCCL communicator cannot be made on ANY rank of the group, every rank falls back to
    TorchComm over the nccl group (decided together: one all-reduce of a flag) and the line says why.  -> (comm, kind)"""
    from hisatgenotype_amd import dist as hdist
    if DIST_DEV != "cuda" and COMM_FORCE != "rccl":
        return hdist.TorchComm(group), "torch-gloo (host control plane)"
    if COMM_FORCE == "torch":
        return hdist.TorchComm(group), "torch-nccl (asked for: --comm torch)"
    import torch
    comm, why = None, ""
    try:
        comm = hdist.RcclComm.from_torch(group)
    except BaseException as e:               # noqa: BLE001 (the fallback must be collective: see the flag below)
        why = repr(e)[:200]
    bad = torch.tensor([0.0 if comm is not None else 1.0], dtype=torch.float64, device=DIST_DEV)
    dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=group)
    if bad.item() > 0:
        if comm is not None:
            comm.close()
        return hdist.TorchComm(group), "torch-nccl (RcclComm could not be created on some rank: %s)" % (why or "another rank")
    return comm, "rccl" if not hdist.RcclComm.lib_path else "rccl entry points over %s" % os.path.basename(hdist.RcclComm.lib_path)


def rccl_stats(reset=False):
    import ctypes as C
    n, snt, rcv = C.c_uint64(), C.c_uint64(), C.c_uint64()
    capi.check(capi.lib().hgx_rccl_stats(C.byref(n), C.byref(snt), C.byref(rcv), C.c_int32(1 if reset else 0)))
    return n.value, snt.value, rcv.value


def _timed(dist, n_steps, body):
    """barrier + sync, `n_steps` x body(), sync + barrier; returns the MAX over ranks of the elapsed seconds."""
    capi.sync()
    if dist is not None:
        _torch_sync()
        dist.barrier()
    t0 = time.perf_counter()
    last = None
    for _ in range(n_steps):
        last = body()
    capi.sync()
    if dist is not None:
        _torch_sync()
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch
        tt = torch.tensor([elapsed], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    return elapsed, last


def run_class1(args, rank, local_rank, world, dist):
    """BASELINE.json configs[2]: HLA class I (A + B + C), 1 M reads each.  Loci are sharded over the GPUs (rank groups in
    proportion to the loci's read counts); a locus that owns several ranks has its PAIRS sharded over them (pileup
    all-reduce at parse time, class tables gathered and merged per step, EMs replicated: dist.type_shard).  A step types all
    three loci once; value = reads of the three loci / time."""
    from hisatgenotype_amd import dist as hdist
    t_setup = time.perf_counter()
    loci = [synth.make_hla_like_locus(gene=g, n_alleles=a, length=ln, n_vars=v, seed=sd, var_id_base=100000 * i)
            for i, (g, a, ln, v, sd) in enumerate(CLASS1)]
    groups = hdist.assign_ranks_to_loci([args.pairs] * len(loci), world)
    comms, comm_kinds = {}, {}
    if dist is not None:                                        # every rank creates every sub-group, in the same order
        force_comm = os.environ.get("HGX_FORCE_DIST") == "comm"       # (tests: the exchange path of a sharded locus with a group of ONE rank)
        for i in sorted(groups):
            if len(groups[i]) > 1 or force_comm:
                g = dist.new_group(groups[i])
                if rank in groups[i]:
                    comms[i], comm_kinds[loci[i].gene] = make_comm(dist, g)
    mine = [i for i in sorted(groups) if rank in groups[i]]
    work = []
    shard_routes, shard_bam, whole_sam = {}, {}, {}
    want_files = world == 1 and dist is None and not args.no_e2e
    file_of, file_dir = {}, None
    if want_files:
        import tempfile
        file_dir = tempfile.mkdtemp(prefix="hgx_class1_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    for i in mine:
        loc = loci[i]
        pl = hl.PackedLocus.from_synth(loc)
        pl.index()
        sample = synth.pick_sample(loc, 101 + i)
        sam = synth.simulate_sam_fast(loc, sample, args.pairs, err_rate=args.err, seed=100 + i)
        if want_files:
            from hisatgenotype_amd import bamio
            fp = os.path.join(file_dir, "%s.bam" % loc.gene)
            bamio.write_bam_native(fp, sam.encode(), [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
            file_of[i] = fp
        if i in comms:
            # this rank's consecutive share of the locus' name-grouped stream through the DEVICE front end; the pileup counters are
            # summed over the rank group where k_fe_pileup left them, in HBM, over RCCL (dist.parse_shard)
            shard_text = hdist.split_name_grouped(sam, len(groups[i]))[groups[i].index(rank)]
            batch, db = hdist.parse_shard(pl, shard_text, comms[i])
            shard_routes[i] = engine.front_last()
            if not args.no_e2e:                                # ... and as a BAM file of its own, for the per-rank file -> result leg
                import tempfile
                from hisatgenotype_amd import bamio
                d_ = tempfile.mkdtemp(prefix="hgx_class1_r%d_" % rank, dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
                shard_bam[i] = os.path.join(d_, "%s.shard%d.bam" % (loc.gene, groups[i].index(rank)))
                bamio.write_bam_native(shard_bam[i], shard_text, [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
            del shard_text
            if args.check_unsharded:
                whole_sam[i] = sam
        else:
            batch = pl.parse_sam(sam)
            db = engine.DeviceBatch(batch)
        del sam
        work.append((i, pl, batch, db, comms.get(i), sample))
    t_setup = time.perf_counter() - t_setup

    # Several whole loci on this rank (always so on one GPU): typed side by side, one host thread and stream set per locus -- the
    # reference's locus loop (typing_core.py:370) has no dependency between loci, and the EM of one locus is a chain of short launches
    # that leaves most of the GPU to the scoring of the next.  (--one-by-one: locus after locus.)
    import threading
    side_by_side = not comms and len(work) > 1 and not args.one_by_one
    pool = {"mode": 0, "stop": False, "res": [None] * len(work), "err": [], "timing": {}}
    if side_by_side:
        pool["start"], pool["done"] = threading.Barrier(len(work) + 1), threading.Barrier(len(work) + 1)
        gate = engine.Gate()

        def worker(k):
            i, pl, batch, db, _, _ = work[k]
            capi.set_device(local_rank)
            capi.set_stream_slot(k)
            st = capi.get_stream(2)
            mode = 0
            while True:
                pool["start"].wait()
                if pool["stop"]:
                    break
                try:
                    if pool["mode"] != mode:
                        mode = pool["mode"]
                        engine.em_set_timing(mode)
                    pool["res"][k] = step(pl, batch, db, None, st, gate)
                    capi.sync(st)
                except BaseException as e:        # re-raised on the main thread
                    pool["err"].append(e)
                pool["done"].wait()
            pool["timing"][k] = engine.em_get_timing()
        threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(len(work))]
        for t in threads:
            t.start()

    def body():
        out = {}
        if side_by_side:
            pool["start"].wait()
            pool["done"].wait()
            if pool["err"]:
                raise pool["err"][0]
            return {w[0]: pool["res"][k] for k, w in enumerate(work)}
        for i, pl, batch, db, comm, sample in work:
            if comm is not None:
                out[i] = hdist.type_shard(pl, batch, db, comm)
            else:
                out[i] = step(pl, batch, db)
        return out
    for _ in range(args.warmup):
        body()
    state = {"k": 0}
    timing = not args.no_kernel_timing and not comms
    n_timed = min(N_TIMED_STEPS, args.steps)

    step_times = []

    def timed_body():
        mode = 2 if (timing and state["k"] >= args.steps - n_timed) else 0
        pool["mode"] = mode
        engine.em_set_timing(mode)
        state["k"] += 1
        t0 = time.perf_counter()
        out = body()
        step_times.append(time.perf_counter() - t0)
        return out
    rccl_stats(reset=True)
    for c in comms.values():
        if hasattr(c, "stats"):
            c.stats = [0, 0, 0]
    elapsed, last = _timed(dist, args.steps, timed_body)
    xs = list(rccl_stats())
    for c in comms.values():
        if hasattr(c, "stats"):
            xs = [a + b for a, b in zip(xs, c.stats)]
    exchange = {"collectives_per_step": xs[0] / max(args.steps, 1), "bytes_sent_per_step": xs[1] // max(args.steps, 1),
                "bytes_received_per_step": xs[2] // max(args.steps, 1), "of": "rank 0's sharded loci (class tables of both levels + totals)"} if comms else None
    st_sorted = sorted(step_times)
    step_spread = {"min": round(st_sorted[0] * 1e3, 3), "median": round(st_sorted[len(st_sorted) // 2] * 1e3, 3), "max": round(st_sorted[-1] * 1e3, 3),
                   "note": "this rank's host-side step times inside the timed region"} if st_sorted else None
    em_timing = engine.em_get_timing() if timing else {}
    engine.em_set_timing(0)
    if side_by_side:
        pool["stop"] = True
        pool["start"].wait()
        for t in threads:
            t.join()
        if timing:                                              # the workers' totals (thread-local in libhgx), added up
            em_timing = {}
            for tm in pool["timing"].values():
                for name, v in tm.items():
                    acc = em_timing.setdefault(name, [0.0, 0, 0, 0])
                    for q in range(4):
                        acc[q] += v[q]
            em_timing = {k: tuple(v) for k, v in em_timing.items()}
    reads = sum(r.num_reads for i, r in last.items() if groups[i][0] == rank)        # every locus counted once
    calls = {loci[i].gene: ([a for a, _ in r.gene_prob[:2]], work[k][5]) for k, (i, r) in enumerate(sorted(last.items()))}
    if dist is not None:
        import torch
        rr = torch.tensor([float(reads)], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(rr, op=dist.ReduceOp.SUM)
        reads = float(rr.item())
        allc = [None] * world
        dist.all_gather_object(allc, calls)
        calls = {g: v for part in allc for g, v in part.items()}
    sharded_ok = None
    if args.check_unsharded and dist is not None:
        import torch
        ok = True
        for i, pl, batch, db, comm, sample in work:
            if comm is not None:
                ref = hgx.type_locus(pl, whole_sam[i])
                r = last[i]
                ok = ok and (r.num_reads, r.num_pairs) == (ref.num_reads, ref.num_pairs) and r.counts_sorted == ref.counts_sorted \
                    and r.em == ref.em and r.gene_prob == ref.gene_prob
        tt = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(tt, op=dist.ReduceOp.MIN)
        sharded_ok = bool(tt.item() > 0.5)
        whole_sam.clear()
    e2e_shards = None
    if dist is not None and not args.no_e2e and (any(len(g) > 1 for g in groups.values()) or (comms and shard_bam)):
        # (EVERY rank enters: the barrier and the reductions below are on the world group; a rank without a sharded locus has no calls to make)
        # sharded loci, files -> result: every rank of a group types its own BAM shard through dist.type_locus_sharded (device
        # inflate / walk / sort, device front end, pileup all-reduce in HBM, class-table all-gather, EMs) -- all ranks at once
        import shutil
        import torch
        try:
            n_calls = 3
            for i, pl, batch, db, comm, sample in work:
                if comm is not None:
                    hdist.type_locus_sharded(pl, None, comm, alignment_file=shard_bam[i], regions=[pl.ref_allele])
            _torch_sync()
            dist.barrier()
            t0 = time.perf_counter()
            ok = True
            for _ in range(n_calls):
                for i, pl, batch, db, comm, sample in work:
                    if comm is not None:
                        r_f = hdist.type_locus_sharded(pl, None, comm, alignment_file=shard_bam[i], regions=[pl.ref_allele])
                        ok = ok and engine.front_last()[0] == 2 and r_f.gene_prob == last[i].gene_prob
            dt = time.perf_counter() - t0
            tt = torch.tensor([dt, 0.0 if ok else 1.0], dtype=torch.float64, device=DIST_DEV)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            e2e_shards = {"input": "every rank of a sharded locus its own coordinate-sorted BAM shard, %d calls, all ranks at once" % n_calls,
                          "ms_per_call": round(float(tt[0].item()) / n_calls * 1e3, 2),
                          "device_front_end_on_every_rank_and_results_identical_to_the_resident_path": bool(tt[1].item() == 0.0)}
        finally:
            for f in shard_bam.values():
                shutil.rmtree(os.path.dirname(f), ignore_errors=True)
    e2e = None
    if want_files:
        # file -> result for the three loci: coordinate-sorted BAM files (as the reference's pipeline stores alignments) through
        # hgx_type_file, locus after locus and side by side (a host thread per locus); the results must be the resident path's
        import shutil
        import threading
        try:
            def files_once(parallel):
                got = {}

                def one(k):
                    i, pl = work[k][0], work[k][1]
                    got[i] = hgx.type_file(pl, file_of[i])
                t0 = time.perf_counter()
                if parallel:
                    ths = [threading.Thread(target=one, args=(k,)) for k in range(len(work))]
                    for t in ths:
                        t.start()
                    for t in ths:
                        t.join()
                else:
                    for k in range(len(work)):
                        one(k)
                return time.perf_counter() - t0, got
            files_once(False)
            seq = sorted(files_once(False)[0] for _ in range(3))
            par_runs = [files_once(True) for _ in range(3)]
            par = sorted(t for t, _ in par_runs)
            got = par_runs[-1][1]
            same = all(got[i].gene_prob == last[i].gene_prob and got[i].num_reads == last[i].num_reads for i in got)
            n_r = sum(r.num_reads for r in got.values())
            e2e = {"input": "three coordinate-sorted BAM files (%.0f MB in all)" % (sum(os.path.getsize(f) for f in file_of.values()) / 1e6),
                   "locus_after_locus_ms": round(seq[1] * 1e3, 2), "side_by_side_ms": round(par[1] * 1e3, 2),
                   "reads_per_s": round(n_r / min(seq[1], par[1]), 1), "result_identical_to_hbm_path": bool(same),
                   "note": "hgx_type_file per locus: the host reads the file and hops through its BGZF container; inflate, record walk, region "
                           "filter, name sort, record fields, filters, key grouping, pileup, decode, piece table, pair protocol and the typing "
                           "path on the GPU (median of 3 after a warm-up)"}
        finally:
            shutil.rmtree(file_dir, ignore_errors=True)
    cb = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        n_cpu = 1500
        cb = cpu_baseline_tasks([(loci[i], synth.simulate_sam_fast(loci[i], work[k][5], n_cpu, err_rate=args.err, seed=100 + i))
                                 for k, (i, *_rest) in enumerate(work)], "%d pairs of each of the three loci (same generator and seeds)" % n_cpu)
    if rank == 0:
        return ({
            "metric": "typed reads/sec at HLA class I (A+B+C, ~7-8k alleles each, 2x150bp)", "value": round(reads * args.steps / elapsed, 1),
            "unit": "reads/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "u64 bitsets, f64 EM", "data": "synthetic",
            "config": {"workload": "configs[2]: HLA class I A+B+C, %d simulated 2x150bp pairs each, piece batches resident in HBM" % args.pairs,
                       "rank_groups": {loci[i].gene: groups[i] for i in sorted(groups)},
                       "calls": {g: {"top2": t, "true": s, "correct": sorted(t) == sorted(s)} for g, (t, s) in calls.items()},
                       "form": "the rank's loci side by side (a host thread and stream set per locus)" if side_by_side else "locus after locus",
                       "parallelism": "loci over rank groups; pairs of a locus over the ranks of its group (device front end per shard with the "
                                      "pileup all-reduce on the counters in HBM at parse, class-table all-gather + merge per step over RCCL); "
                                      "no other data-path collective",
                       "front_end_route_of_my_shards": {loci[i].gene: list(r) for i, r in shard_routes.items()},
                       "comm_kind": comm_kinds or None, "exchange": exchange, "sharded_equals_unsharded": sharded_ok,
                       "shared_gpu": bool(args.share_gpu),
                       "e2e_shards": e2e_shards,
                       "setup_s": round(t_setup, 1)},
            "roofline": em_roofline(em_timing, n_timed) if timing else None, "cpu_baseline": cb, "e2e": e2e,
            "stream_sets": engine.stream_sets_info(), "ms_per_step_spread": step_spread})
    return None


def run_dropin(args, name):
    """The drop-in itself, timed: a committed fixture recorded from the REAL reference (tests/golden/<name>.json.gz:
    BASELINE configs[0] = HLA-A-like, 7 000 alleles, 10 k reads, which the reference needed 109 s for; configs[4]'s shape = one CODIS
    STR ladder, 10 k reads) through `hisatgenotype_amd.typing(<the reference's 38 arguments>)` -> report file, and through
    `genotyping_locus(<32 arguments>)` from index files on disk.  Wall time per call with the split typing() records (locus packing,
    index upload + pattern tables, file read + front end, GPU typing + result, report), first call and repeated calls (the
    reference's own shape: one typing() per sample on one index), report text `==` the reference's recorded report."""
    import copy
    import gzip
    import shutil
    import tempfile
    from hisatgenotype_amd import locus as hlocus
    with gzip.open(os.path.join(ROOT, "tests", "golden", name + ".json.gz"), "rb") as f:
        fx = json.loads(f.read().decode())
    loc = synth.Locus.from_json(fx["locus"]) if fx["locus"] is not None else synth.make_hla_like_locus(**fx["locus_params"])
    o = fx["options"]
    keep = lambda ls: [l for l in ls if "aligned" in l or "ranked" in l or "(count:" in l]
    want = keep(fx["report"].split("\n"))
    tmp = tempfile.mkdtemp(prefix="hgx_dropin_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        sam_path = os.path.join(tmp, "sample.sam")
        with open(sam_path, "w") as f:
            f.write(fx["sam"])
        d = loc.reference_dicts()
        base = loc.base_fname
        rep_path = os.path.join(tmp, "assembly_graph-%s.sample.report" % base)

        def call(dd):
            t0 = time.perf_counter()
            hgx.typing(False, os.path.join(tmp, base), [loc.gene], "", True, set(), dd["refGenes"], dd["Genes"], dd["Gene_names"],
                       dd["Gene_lengths"], dd["refGene_loci"], dd["Vars"], dd["Var_list"], dd["Links"], [["hisat2", "graph"]], o["num_editdist"],
                       False, "assembly_graph", o["error_correction"], True, o["allow_discordant"], False, o["remove_low"], [], False,
                       ["sample.fq"], sam_path, [], o["read_len"], o["frag_len"], 1, False, 0, False, tmp, "NONE", True, 0)
            dt = time.perf_counter() - t0
            prof = dict(htyping.last_profile[0])
            with open(rep_path) as f:
                same = keep(f.read().split("\n")) == want
            return dt, prof, same

        def fmt(p):
            return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in p.items() if k != "gene"}
        hlocus.LOCUS_CACHE.clear()
        t_first, p_first, ok_first = call(d)                               # first call of the process on this index: packs, uploads
        rest = sorted((call(d) for _ in range(7)), key=lambda r: r[0])
        t_rep, p_rep, ok_rep = rest[len(rest) // 2]
        t_copy, p_copy, ok_copy = call(copy.deepcopy(d))                   # equal dicts in other objects (re-read index): content key
        htyping.typing_options.em_fast = True                              # the other EM arithmetic (table lookups, <= 1e-8; bar 1e-5)
        try:
            fast = sorted((call(d) for _ in range(5)), key=lambda r: r[0])[2]
        finally:
            htyping.typing_options.em_fast = False
        hits = (hlocus.LOCUS_CACHE.hits_identity, hlocus.LOCUS_CACHE.hits_content, hlocus.LOCUS_CACHE.misses)
        # the same through genotyping_locus from index files on disk (driver.py; typing_core.py:2278-2691)
        ix_dir = os.path.join(tmp, "ix")
        synth.write_index([loc], ix_dir, base)

        def call_gl():
            t0 = time.perf_counter()
            hgx.genotyping_locus(base, [loc.gene], "", ix_dir, [], True, [["hisat2", "graph"]], ["sample.fq"], True, sam_path, 1, 10,
                                 o["read_len"], o["frag_len"], False, o["num_editdist"], 0.0, 0.0, [], False, "assembly_graph",
                                 o["error_correction"], True, o["allow_discordant"], False, o["remove_low"], [], 0, False, tmp, True, {})
            dt = time.perf_counter() - t0
            with open(rep_path) as f:
                same = keep(f.read().split("\n")) == want
            return dt, dict(htyping.last_profile[0]), same
        import io
        import contextlib
        with contextlib.redirect_stderr(io.StringIO()):                    # (genotyping_locus prints the locus list like the reference)
            g_first = call_gl()
            g_rest = sorted((call_gl() for _ in range(5)), key=lambda r: r[0])
        g_rep = g_rest[len(g_rest) // 2]
        n_rec = fx["reference_timing"]["sam_records"]
        ref_s = fx["reference_timing"]["seconds"]
        return {
            "metric": "wall time of one typing() call (file -> report), the reference's own entry point", "unit": "ms", "higher_is_better": False,
            "value": round(t_rep * 1e3, 2),
            "config": {"workload": "%s: tests/golden/%s.json.gz (%d SAM records, %d alleles), the input the real reference was timed on" % (
                "configs[0]" if name == "hla_7000_10k" else "configs[4] shape", name, n_rec, len(loc.allele_names) - 1),
                "entry": "hisatgenotype_amd.typing(<38 arguments of typing_core.py:249-286>) -> <out_dir>/assembly_graph-%s.sample.report" % base},
            "report_identical_to_the_reference": bool(ok_first and ok_rep and ok_copy and g_first[2] and g_rep[2]),
            "first_call_ms": round(t_first * 1e3, 2), "first_call_split_ms": fmt(p_first),
            "repeated_call_ms": round(t_rep * 1e3, 2), "repeated_call_split_ms": fmt(p_rep),
            "equal_dicts_in_new_objects_ms": round(t_copy * 1e3, 2), "equal_dicts_split_ms": fmt(p_copy),
            "em_arithmetic": "default of typing(): the reference's order of floating-point operations (abundances == the reference's doubles)",
            "repeated_call_table_lookup_em_ms": round(fast[0] * 1e3, 2), "table_lookup_em_report_identical": bool(fast[2]),
            "locus_cache": {"identity_hits": hits[0], "content_hits": hits[1], "misses": hits[2]},
            "genotyping_locus": {"entry": "hisatgenotype_amd.genotyping_locus(<32 arguments of typing_core.py:2278-2309>) on index files on disk",
                                 "first_call_ms": round(g_first[0] * 1e3, 2), "repeated_call_ms": round(g_rep[0] * 1e3, 2),
                                 "repeated_call_split_ms": fmt(g_rep[1])},
            "reads_per_s_repeated": round(n_rec / t_rep, 1),
            "reference_recorded": {"seconds": ref_s, "records_per_s": fx["reference_timing"]["records_per_s"], "cpu": fx["reference_timing"]["cpu"],
                                   "what": fx["reference_timing"]["what"], "note": "recorded on the build container (tests/golden/make_golden.py), not on this box"},
            "speedup_over_the_recorded_reference": {"first_call": round(ref_s / t_first, 1), "repeated_call": round(ref_s / t_rep, 1)},
        }
    finally:
        shutil.rmtree(tmp, ignore_errors=True)



def run_sample6(args):
    """ONE sample x SIX loci at real depth (the reference's call shape: typing() loops its locus_list over one
    alignment file, typing_core.py:370, 436-468): the HLA panel's six loci, 3 000 read pairs each, in ONE coordinate-sorted BAM ->
    `hisatgenotype_amd.typing(<38 arguments>, locus_list = the six genes)` -> one report with six sections.  The file is read and
    inflated once (hgx_alignment_open), every locus goes through the device front end (k_fe_*: 6 000 records are above the 1 000-record
    gate of round 6; rounds 3-5 sent them to the host stages) and the loci are typed side by side."""
    import shutil
    import tempfile
    from hisatgenotype_amd import bamio, locus as hlocus
    n_pairs = 3000
    loci = [synth.make_hla_like_locus(gene=g, n_alleles=a, length=ln, n_vars=v, seed=500 + i, var_id_base=10000 * i)
            for i, (g, a, ln, v) in enumerate(PANEL)]
    samples = [synth.pick_sample(loc, 7000 + k) for k, loc in enumerate(loci)]
    sams = [synth.simulate_sam_fast(loc, smp, n_pairs, err_rate=args.err, seed=900 + k) for k, (loc, smp) in enumerate(zip(loci, samples))]
    d = {k: {} for k in ("refGenes", "Genes", "Gene_names", "Gene_lengths", "refGene_loci", "Vars", "Var_list", "Links")}
    for loc in loci:
        for k, v in loc.reference_dicts().items():
            d[k].update(v)
    genes = [loc.gene for loc in loci]
    tmp = tempfile.mkdtemp(prefix="hgx_sample6_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bam = os.path.join(tmp, "sample.bam")
        bamio.write_bam_native(bam, "".join(sams).encode(), [(loc.ref_allele, len(loc.backbone)) for loc in loci], sort_by_coordinate=True)
        rep_path = os.path.join(tmp, "assembly_graph-hla.sample.report")

        def call(side_by_side=True, em_fast=False, together=False):
            htyping.typing_options.loci_side_by_side, htyping.typing_options.em_fast = side_by_side, em_fast
            htyping.typing_options.loci_together = together
            try:
                t0 = time.perf_counter()
                hgx.typing(False, os.path.join(tmp, "hla"), genes, "", True, set(), d["refGenes"], d["Genes"], d["Gene_names"], d["Gene_lengths"],
                           d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"], [["hisat2", "graph"]], 2, False, "assembly_graph", True, True,
                           False, False, True, [], False, ["sample.fq"], bam, [], 150, 400, 1, False, 0, False, tmp, "NONE", False, 0)
                dt = time.perf_counter() - t0
            finally:
                htyping.typing_options.loci_side_by_side, htyping.typing_options.em_fast, htyping.typing_options.loci_together = True, False, False
            with open(rep_path) as f:
                rep = f.read()
            return dt, [dict(p) for p in htyping.last_profile], rep
        hlocus.LOCUS_CACHE.clear()
        t_first, _, rep0 = call()
        cl0 = engine.emx_cluster_stats()
        runs = sorted((call() for _ in range(5)), key=lambda r: r[0])
        cl1 = engine.emx_cluster_stats()
        t_rep, prof, rep = runs[len(runs) // 2]
        engine.test_switch("emx_cluster_lone", "0")           # the loci's EM #1 on one workgroup each (rounds 3-5's form), for comparison
        try:
            t_nocl = sorted(call()[0] for _ in range(3))[1]
        finally:
            engine.test_switch("emx_cluster_lone", None)
        t_seq = sorted(call(side_by_side=False)[0] for _ in range(3))[1]
        t_fast = sorted(call(em_fast=True)[0] for _ in range(3))[1]
        tog = sorted((call(together=True) for _ in range(3)), key=lambda r: r[0])[1]
        # the old way: one hgx_type_file per locus (the file read and inflated six times), locus after locus
        pls = [hlocus.PackedLocus.cached_from_reference_dicts(g, "hla", d["refGenes"], d["Genes"], d["Gene_names"], d["Gene_lengths"], d["refGene_loci"],
                                                              d["Vars"], d["Var_list"], d["Links"]) for g in genes]

        def per_locus_files():
            t0 = time.perf_counter()
            out = [hgx.type_file(pl, bam, regions=[pl.ref_allele]) for pl in pls]
            return time.perf_counter() - t0, out
        per_locus_files()
        t_old, res_old = sorted((per_locus_files() for _ in range(3)), key=lambda r: r[0])[1]
        # every section of the report against the locus typed alone from its own SAM text
        keep = lambda ls: [l for l in ls if "aligned" in l or "ranked" in l or "(count:" in l]
        want = []
        for pl, sam in zip(pls, sams):
            lines, _ = hgx.report_lines(hgx.type_locus(pl, sam), False, (), False)
            want += keep(lines)
        top2 = {}
        for pl, r in zip(pls, res_old):
            top2[pl.gene] = [a for a, _ in r.gene_prob[:2]]
        return {
            "metric": "wall time of one typing() call over ONE sample x 6 loci (file -> six report sections)", "unit": "ms", "higher_is_better": False,
            "value": round(t_rep * 1e3, 2),
            "config": {"workload": "1 sample x 6 loci (%s alleles), %d simulated 2x150bp pairs per locus in ONE coordinate-sorted BAM (%.1f MB)" % (
                "/".join(str(p[1]) for p in PANEL), n_pairs, os.path.getsize(bam) / 1e6),
                "entry": "hisatgenotype_amd.typing(<38 arguments>, locus_list = %s)" % genes},
            "reads_per_s": round(2 * n_pairs * len(loci) / t_rep, 1),
            "first_call_ms": round(t_first * 1e3, 2), "repeated_call_ms": round(t_rep * 1e3, 2),
            "all_five_repeated_calls_ms": [round(r[0] * 1e3, 2) for r in runs],
            "emx_cluster_problems_and_fallbacks_in_those_calls": [cl1[0] - cl0[0], cl1[1] - cl0[1]],
            "reference_order_em_on_one_workgroup_per_locus_ms": round(t_nocl * 1e3, 2),
            "loci_one_after_the_other_ms": round(t_seq * 1e3, 2), "table_lookup_em_ms": round(t_fast * 1e3, 2),
            "one_hgx_type_file_per_locus_ms": round(t_old * 1e3, 2),
            "front_end_route_per_locus": {p["gene"]: p["front_end_route"] for p in prof},
            "alignment_open_ms": round(prof[0].get("alignment_open_ms_shared", 0.0), 3),
            "per_locus_ms": {p["gene"]: {"file_region_and_front_end": round(p["file_read_and_front_end_ms"], 3),
                                         "gpu_typing_and_result": round(p["gpu_typing_and_result_ms"], 3)} for p in prof},
            "loci_parsed_side_by_side_then_typed_by_one_hgx_type_many_loci_call_ms": round(tog[0] * 1e3, 2),
            "that_form_s_report_identical": keep(tog[2].split("\n")) == want,
            "report_sections_identical_to_the_loci_typed_alone": keep(rep.split("\n")) == want and keep(rep0.split("\n")) == want,
            "calls": {loc.gene: {"top2": top2[loc.gene], "true": smp, "correct": sorted(top2[loc.gene]) == sorted(smp)} for loc, smp in zip(loci, samples)},
        }
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_panel64(args, rank, local_rank, world, dist):
    """BASELINE.json configs[3]: the full HLA panel (A, B, C, DRB1, DQA1, DQB1) x 64 synthetic samples = 384 independent
    (sample, locus) tasks, split over the GPUs by dist.shard (greedy by allele count; no data-path collective).  A step types
    every task of the rank once from its resident piece batch; value = reads of all tasks / time (max over ranks)."""
    from hisatgenotype_amd import dist as hdist
    t_setup = time.perf_counter()
    loci = [synth.make_hla_like_locus(gene=g, n_alleles=a, length=ln, n_vars=v, seed=500 + i, var_id_base=10000 * i)
            for i, (g, a, ln, v) in enumerate(PANEL)]
    tasks = [(s, k) for s in range(64) for k in range(len(loci))]
    mine = hdist.shard(tasks, rank, world, [len(loci[k].allele_names) for _, k in tasks])
    packed = {}
    work = []
    want_files = world == 1 and dist is None and not args.no_e2e and not args.one_by_one
    file_of, file_dir = {}, None
    if want_files:
        import tempfile
        from hisatgenotype_amd import bamio
        file_dir = tempfile.mkdtemp(prefix="hgx_panel_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    for s, k in mine:
        if k not in packed:
            packed[k] = hl.PackedLocus.from_synth(loci[k])
            packed[k].index()
        sample = synth.pick_sample(loci[k], 1000 * s + k)
        sam = synth.simulate_sam_fast(loci[k], sample, args.panel_pairs, err_rate=args.err, seed=100 * s + k)
        if want_files:
            fp = os.path.join(file_dir, "s%02d_%s.bam" % (s, loci[k].gene))
            bamio.write_bam_native(fp, sam.encode(), [(loci[k].ref_allele, len(loci[k].backbone))], sort_by_coordinate=True)
            file_of[(s, k)] = fp
        batch = packed[k].parse_sam(sam)
        work.append((s, k, batch, engine.DeviceBatch(batch), sample))
    # the rank's tasks of a locus, merged and resident in HBM: ONE launch chain per locus (hgx_type_many)
    manies = {}
    if not args.one_by_one:
        for k in sorted(packed):
            idx = [n for n, w in enumerate(work) if w[1] == k]
            manies[k] = (idx, engine.ManyBatch(packed[k], [work[n][2] for n in idx]))
    t_setup = time.perf_counter() - t_setup
    inflight = max(1, args.inflight)

    def body():
        import threading
        out = [None] * len(work)
        if manies:
            ks = sorted(manies)
            rows = htyping.type_many_loci([packed[k] for k in ks], [manies[k][1] for k in ks], light=True, em_fast=False if args.em_exact else None)
            for k, row in zip(ks, rows):
                for n, r in zip(manies[k][0], row):
                    out[n] = r
            return out
        if inflight <= 1:
            for n, (s, k, batch, db, _) in enumerate(work):
                out[n] = step(packed[k], batch, db)
            return out
        nxt, lock, gate, errs = [0], threading.Lock(), engine.Gate(), []

        def worker(slot):
            try:
                capi.set_device(local_rank)
                capi.set_stream_slot(slot)
                st = capi.get_stream(2)
                while True:
                    with lock:
                        n = nxt[0]
                        nxt[0] += 1
                    if n >= len(work):
                        return
                    s, k, batch, db, _ = work[n]
                    out[n] = step(packed[k], batch, db, None, st, gate)
            except BaseException as e:
                errs.append(e)
        ths = [threading.Thread(target=worker, args=(i,)) for i in range(inflight)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errs:
            raise errs[0]
        return out
    for _ in range(args.warmup):
        body()
    timing = bool(manies) and not args.no_kernel_timing
    if timing:
        engine.emx_set_timing(True)
    elapsed, last = _timed(dist, args.steps, body)
    emx = None
    if timing:
        engine.emx_set_timing(False)
        emx = {"table lookups" if f else "reference order": engine.emx_get_timing(f) for f in (1, 0)}
    if manies:
        reads = float(sum(r[0] for r in last))
        correct = sum(1 for r, (s, k, _, _, sample) in zip(last, work) if sorted(r[1]) == sorted(sample))
    else:
        reads = float(sum(r.num_reads for r in last))
        correct = sum(1 for r, (s, k, _, _, sample) in zip(last, work) if sorted(a for a, _ in r.gene_prob[:2]) == sorted(sample))
    n_tasks = len(work)
    if dist is not None:
        import torch
        rr = torch.tensor([reads, float(correct), float(n_tasks)], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(rr, op=dist.ReduceOp.SUM)
        reads, correct, n_tasks = float(rr[0].item()), int(rr[1].item()), int(rr[2].item())
    roof = None
    if emx:
        kernels = {}
        for name, (ms, nl, nj, na, nb) in emx.items():
            if nl:
                kernels["k_emx (%s)" % name] = {
                    "launches": nl, "jobs_per_launch": nj // nl, "em_map_applications_per_launch": na // nl, "alg_bytes_per_launch": int(nb // nl),
                    "avg_ms": round(ms / nl, 4), "total_ms_per_step": round(ms / args.steps, 4), "GBps": round(nb / (ms * 1e-3) / 1e9, 1),
                    "bound": "hbm", "peak_GBps": HBM_PEAK_GBS, "frac": round(nb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        if kernels:
            dom = max(kernels, key=lambda k: kernels[k]["total_ms_per_step"])
            traffic = None
            try:                                                   # PMC passes of the panel64 command (profiles/README.md)
                traffic = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["hbm_bytes_per_launch"].get(dom)
            except Exception:
                traffic = None
            roof = {"bound": "hbm", "kernel": dom, "achieved": kernels[dom]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": kernels[dom]["frac"],
                    "traffic": traffic, "alg_bytes_per_launch": kernels[dom]["alg_bytes_per_launch"], "avg_launch_ms": kernels[dom]["avg_ms"],
                    "note": "the one-workgroup-per-task EM kernel (EM #1 of all tasks in one launch; EM #2 in another): HIP events around every "
                            "launch of the timed region; algorithmic bytes per launch = sum over its jobs of applications x (C * A' / 8 + 16 A' + "
                            "16 C) (SURVEY.md 8d).  The kernel is bound by the LDS pipe of ONE CU per task, not by HBM: a pass makes one 8-byte table "
                            "lookup per 8 matrix bits, i.e. 2 C A' bytes of LDS reads per application -- alone on a CU a 1 600 x 4 549 problem "
                            "reads 14.6 MB per application in 89 us = 164 GB/s = 0.56 of a CU's 293 GB/s (tools/emx_timing.py) -- and the launch "
                            "ends with its longest problem (3-13 EM iterations per task).  The HBM fraction says how far a task-parallel EM sits "
                            "from streaming its matrices",
                    "kernels": kernels}
    # the same panel with the OTHER EM arithmetic, a few steps outside the timed region: the line then carries both the throughput
    # form (table lookups, <= 1e-8) and the bit-identical form (the library's default, hgx_type_opts.em_fast = 0)
    other = None
    if manies and world == 1:
        ks = sorted(manies)
        t0 = time.perf_counter()
        n_other = 3
        for _ in range(n_other):
            rows_o = htyping.type_many_loci([packed[k] for k in ks], [manies[k][1] for k in ks], light=True, em_fast=None if args.em_exact else False)
        dt = (time.perf_counter() - t0) / n_other
        same = sum(1 for k, row in zip(ks, rows_o) for n, r in zip(manies[k][0], row) if sorted(r[1]) == sorted(last[n][1]))
        other = {"em_arithmetic": "table lookups (the many-task calls' default)" if args.em_exact else "reference order (hgx_type_opts.em_fast = 2: bit-identical abundances)",
                 "ms_per_step": round(dt * 1e3, 3), "value": round(reads / dt, 1), "steps": n_other, "tasks_with_the_same_top2_as_the_timed_form": same}
    e2e = None
    if want_files and manies:
        # 384 files -> 384 results (the loop of /root/reference/hisatgenotype:613-665 over samples x loci): per locus ONE pass of the
        # device front end over its 64 samples' files (hgx_many_create_files: the files read side by side on host threads, every
        # record carries its task), the loci side by side; then hgx_type_many_loci as in the timed step.  Beside it, once, round
        # 3's form: the host front end per file, then hgx_many_create's merge + upload.
        import shutil
        from concurrent.futures import ThreadPoolExecutor
        try:
            nthr = max(4, int(2 * (cgroup_cpu_quota() or (os.cpu_count() or 8))))
            ks = sorted(manies)
            paths_of = {k: [file_of[(work[n][0], k)] for n in manies[k][0]] for k in ks}

            def files_once(device=True):
                t0 = time.perf_counter()
                routes = None
                if device:
                    def one(k):
                        capi.set_stream_slot(("panel files", k))              # a stream per locus: its uploads and kernels beside the others'
                        m = engine.ManyBatch.from_files(packed[k], paths_of[k], regions=[packed[k].ref_allele] * len(paths_of[k]),
                                                        n_threads=max(2, nthr // 3), stream=capi.get_stream(1))
                        return m, engine.front_last(), engine.front_last_bytes()
                    with ThreadPoolExecutor(len(ks)) as ex:
                        got = list(ex.map(one, ks))
                    mbs = [g[0] for g in got]
                    routes = [(g[1], g[2]) for g in got]
                    t1 = t2 = time.perf_counter()
                else:
                    with ThreadPoolExecutor(nthr) as ex:
                        futs = {k: [ex.submit(packed[k].parse_alignment_file, fp, [packed[k].ref_allele], n_threads=1) for fp in paths_of[k]] for k in ks}
                        got_b = {k: [f.result() for f in futs[k]] for k in ks}
                    t1 = time.perf_counter()
                    mbs = [engine.ManyBatch(packed[k], got_b[k]) for k in ks]
                    t2 = time.perf_counter()
                rows_f = htyping.type_many_loci([packed[k] for k in ks], mbs, light=True, em_fast=False if args.em_exact else None)
                t3 = time.perf_counter()
                dims = [(m.n_pieces, m.n_pairs, m.n_refs, m.n_reads, tuple(m.task_reads), tuple(m.task_pieces)) for m in mbs]
                for m in mbs:
                    m.close()
                return (t3 - t0, t1 - t0, t2 - t1, t3 - t2), {k: row for k, row in zip(ks, rows_f)}, routes, dims
            files_once()
            runs = [files_once() for _ in range(3)]
            runs.sort(key=lambda r: r[0][0])
            (tot, t_fe, _, t_gpu), rows_f, routes, dims = runs[1]
            files_once(False)
            (tot_h, t_fe_h, t_merge_h, t_gpu_h), rows_h, _, dims_h = files_once(False)
            same = sum(1 for k in rows_f for n, r in zip(manies[k][0], rows_f[k]) if sorted(r[1]) == sorted(last[n][1]) and r[0] == last[n][0])
            e2e = {"input": "%d coordinate-sorted BAM files of %d pairs (%.0f MB in all)" % (len(file_of), args.panel_pairs,
                                                                                               sum(os.path.getsize(f) for f in file_of.values()) / 1e6),
                   "ms": round(tot * 1e3, 1), "reads_per_s": round(reads / tot, 1),
                   "stages_ms": {"hgx_many_create_files, %d loci side by side (the host reads the files; BGZF inflate, record walk / filter / name sort, records -> merged batch on the device)" % len(ks):
                                 round(t_fe * 1e3, 1), "hgx_type_many_loci": round(t_gpu * 1e3, 1)},
                   "front_end": {"route_and_decline_code_per_locus": [list(r[0]) for r in routes], "bytes_to_device": sum(r[1] for r in routes)},
                   "tasks_with_the_timed_step_s_reads_and_top2": same,
                   "merged_batches_identical_to_the_host_front_ends": dims == dims_h and all(rows_f[k] == rows_h[k] for k in rows_f),
                   "host_front_ends_instead": {"ms": round(tot_h * 1e3, 1),
                                               "stages_ms": {"front ends of the files (host stages, %d threads)" % nthr: round(t_fe_h * 1e3, 1),
                                                             "merge + upload (hgx_many_create)": round(t_merge_h * 1e3, 1),
                                                             "hgx_type_many_loci": round(t_gpu_h * 1e3, 1)}},
                   "note": "files -> results for the whole panel (median of 3 after a warm-up): the samples of a locus go through ONE pass "
                           "of the device front end (a task alone, 10 000 records, is below its size gate; 64 together are not)"}
        finally:
            shutil.rmtree(file_dir, ignore_errors=True)
    cb = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        n_cpu = 1000
        cb = cpu_baseline_tasks([(loci[k], synth.simulate_sam_fast(loci[k], synth.pick_sample(loci[k], k), n_cpu, err_rate=args.err, seed=k))
                                 for k in range(len(loci))], "sample 0's six tasks at %d pairs each (same generator and seeds)" % n_cpu)
    if rank == 0:
        return ({
            "metric": "typed reads/sec over the HLA panel (6 loci x 64 samples, 2x150bp)", "value": round(reads * args.steps / elapsed, 1),
            "unit": "reads/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "u64 bitsets, f64 EM", "data": "synthetic",
            "config": {"workload": "configs[3]: 6 loci (500-8000 alleles) x 64 samples = %d tasks of %d pairs, piece batches resident in HBM" % (
                n_tasks, args.panel_pairs),
                "tasks_with_both_true_alleles_on_top": correct, "tasks": n_tasks, "samples_in_flight_per_gpu": inflight,
                "form": "one launch chain per task" if args.one_by_one else "hgx_type_many_loci: one launch chain per locus (all its samples together), the EMs of all loci in one launch",
                "em_arithmetic": ("reference order (hgx_type_opts.em_fast = 2: bit-identical)" if args.em_exact else
                                  "the library's default for hgx_type_many_loci: table lookups (abundances within 1e-8 of the reference; bar 1e-5)") if not args.one_by_one else "default",
                "parallelism": "(sample, locus) tasks over GPUs by dist.shard (greedy by allele count), no data-path collective",
                "merged_batches": {packed[k].gene: {"alleles": packed[k].n_alleles, "tasks": m.n_tasks, "pairs": m.n_pairs, "piece_refs": m.n_refs,
                                                    "distinct_pieces": m.n_pieces} for k, (_, m) in sorted(manies.items())},
                "setup_s": round(t_setup, 1)},
            "roofline": roof, "cpu_baseline": cb, "other_em_arithmetic": other, "e2e": e2e, "stream_sets": engine.stream_sets_info()})
    return None


def main():
    args = parse_args()
    if args.e2e_child:
        _e2e_child(args.e2e_child)
        return
    global EM_MODE
    EM_MODE = -1 if args.em_exact else False
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    use_dist = world > 1 or bool(os.environ.get("HGX_FORCE_DIST"))     # the latter exercises the RCCL path on one GPU
    if args.dry_run:
        # launcher check: the ranks meet, agree on the world size, and rank 0 reports what it saw
        seen = world
        if use_dist:
            import torch
            import torch.distributed as dist
            dist.init_process_group(args.backend)
            t = torch.ones(1, dtype=torch.int64)
            if args.backend == "nccl":
                torch.cuda.set_device(local_rank)
                t = t.cuda()
            dist.all_reduce(t)
            seen = int(t.item())
            assert dist.get_world_size() == world
            dist.barrier()
            if args.workload != "class1":
                dist.destroy_process_group()
        line = {"dry_run": True, "n_gpus": seen, "world_size": world, "backend": args.backend, "gpus_arg": args.gpus}
        if args.workload == "class1":
            # the rank groups configs[2] would run with (dist.assign_ranks_to_loci: every rank computes them; they must agree)
            from hisatgenotype_amd import dist as hdist
            groups = hdist.assign_ranks_to_loci([args.pairs] * len(CLASS1), world)
            line["rank_groups"] = {CLASS1[i][0]: groups[i] for i in sorted(groups)}
            line["my_loci_agree"] = True
            if use_dist:
                import torch.distributed as dist
                got = [None] * world
                dist.all_gather_object(got, {k: v for k, v in line["rank_groups"].items()})
                line["my_loci_agree"] = all(g == got[0] for g in got)
                covered = sorted(r for v in got[0].values() for r in v)
                line["every_rank_has_work"] = covered == list(range(world)) or world <= len(CLASS1)
                dist.barrier()
                dist.destroy_process_group()
        if rank == 0:
            print(json.dumps(line))
        return
    if args.gpus != world:
        sys.exit("bench.py: --gpus %d but %d rank(s) are running" % (args.gpus, world))
    global DIST_DEV, COMM_FORCE
    COMM_FORCE = args.comm
    if os.environ.get("HGX_BENCH_RCCL_LIB"):
        from hisatgenotype_amd import dist as hdist_
        hdist_.RcclComm.lib_path = os.environ["HGX_BENCH_RCCL_LIB"]
    dev_id = 0 if args.share_gpu else local_rank          # --share-gpu: every rank on GPU 0 (the multi-rank body on a one-GPU box)
    if use_dist:
        import torch
        import torch.distributed as dist
        if args.backend == "nccl":
            if args.share_gpu:
                sys.exit("bench.py: --share-gpu needs --backend gloo (RCCL refuses two ranks on one device)")
            torch.cuda.set_device(dev_id)
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_id))
        else:
            DIST_DEV = "cpu"                              # control plane over gloo; the data path stays on the GPU
            dist.init_process_group("gloo")
        assert dist.get_world_size() == world
    pre = None
    if (args.full and args.workload == "configs1" and world == 1 and not use_dist and not args.no_e2e and not args.no_cpu_baseline
            and args.e2e_procs.strip()):
        # the N-process host-scaling leg comes FIRST: its children start before this process has touched the GPU.  The sample
        # it makes is the one the rest of the run uses.
        loc0 = synth.make_hla_like_locus(n_alleles=args.alleles, n_vars=args.vars, seed=101)
        sam0 = synth.simulate_sam_fast(loc0, synth.pick_sample(loc0, 101), args.pairs, err_rate=args.err, seed=100)
        procs = [int(x) for x in args.e2e_procs.split(",") if x.strip()]
        try:
            scaling = e2e_scaling(loc0, sam0, procs)
        except Exception as e:                                      # (the leg must not cost the run its headline)
            scaling = {"error": repr(e)[:500]}
        pre = (loc0, sam0, scaling)
    if os.environ.get("HGX_STREAMS"):                     # A/B of the stream placement (tools: "unplaced" = creation order, no probes)
        engine.test_switch("streams", os.environ["HGX_STREAMS"])
    capi.set_device(dev_id)
    local_rank = dev_id                                   # (everything below addresses the GPU through this)
    if args.workload in ("config0_dropin", "codis_dropin", "sample6"):
        if world != 1:
            sys.exit("bench.py: the drop-in legs are one-process measurements")
        print(json.dumps(run_sample6(args) if args.workload == "sample6" else
                         run_dropin(args, "hla_7000_10k" if args.workload == "config0_dropin" else "codis_10k")))
        return
    if args.workload != "configs1":
        line = (run_class1 if args.workload == "class1" else run_panel64)(args, rank, local_rank, world, dist)
        if rank == 0:
            print(json.dumps(line))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- set-up (untimed): locus, index broadcast, reads, front-end, upload --------------------------------
    t_setup = time.perf_counter()
    loc = pre[0] if pre else synth.make_hla_like_locus(n_alleles=args.alleles, n_vars=args.vars, seed=101)
    pl = hl.PackedLocus.from_synth(loc)
    comm_kind, bcast_bytes = None, None
    if use_dist:
        # rank 0's packed link matrix reaches every GPU over RCCL / xGMI: torch.distributed.broadcast on a tensor that ALIASES the index'
        # device block (device to device, in place; dist.broadcast_index).  The weak-scaling line needs nothing else from the fabric, so
        # it stays on torch's own communicator -- the one multi-GPU path of this repository that PyTorch itself exercises everywhere;
        # this library's own ncclComm_t (dist.RcclComm: hgx_index_broadcast, hgx_classes_allgather, ...) carries the per-step
        # exchanges of --workload class1, where a host bounce per step would be the measurement (make_comm)
        from hisatgenotype_amd import dist as hdist
        bcast_bytes = hdist.broadcast_index(pl, src=0)
        comm_kind = "torch-nccl broadcast into the index' device block" if DIST_DEV == "cuda" else "torch-gloo (host control plane)"
    else:
        pl.index()
    sample = synth.pick_sample(loc, 101 + rank)
    sam = pre[1] if pre else synth.simulate_sam_fast(loc, sample, args.pairs, err_rate=args.err, seed=100 + rank)
    batch, t_parse, fe_same = None, None, None
    if args.full:
        t0 = time.perf_counter()
        batch = pl.parse_sam(sam)                           # host front end: the pinned checker of the device front end
        t_parse = time.perf_counter() - t0
    # the batch the timed steps read is the one the DEVICE front end builds in HBM (record route); it must be the host's, byte for byte
    pl.parse_sam_dev(sam).close()                           # (warm-up: staging memory, locus tables)
    t0 = time.perf_counter()
    db = pl.parse_sam_dev(sam)
    t_parse_dev = time.perf_counter() - t0
    fe_route, fe_code = engine.front_last()
    if batch is not None:
        hb = db.to_host()
        fe_same = all(getattr(hb, k).tobytes() == getattr(batch, k).tobytes() for k in ("pieces", "masks", "pair_off", "pair_ref")) and \
            hb.n_reads == batch.n_reads
        del hb
    inflight = max(1, args.inflight)
    if rank != 0 or args.no_cpu_baseline or use_dist or not args.full:
        sam_keep = None
    else:
        sam_keep = sam
    rank_bam = None
    if use_dist and args.full and not args.no_e2e:
        # every rank's own sample as a coordinate-sorted BAM file: the file -> result leg of the N-GPU line (below)
        import tempfile
        from hisatgenotype_amd import bamio
        rank_dir = tempfile.mkdtemp(prefix="hgx_rank%d_" % rank, dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        rank_bam = os.path.join(rank_dir, "reads.bam")
        bamio.write_bam_native(rank_bam, sam.encode(), [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
    del sam
    t_setup = time.perf_counter() - t_setup

    run_steps(pl, batch, db, inflight, max(args.warmup, inflight if args.warmup else 0), None, False, local_rank)
    capi.sync()
    if dist is not None:
        dist.barrier()
    ev = [(capi.Event(), capi.Event(), capi.Event(), capi.Event()) for _ in range(args.steps)]
    timing = not args.no_kernel_timing                     # HIP events around a sample of the EM mat-vec launches
    t0 = time.perf_counter()
    res, t_em, n_em_iter, em_timing = run_steps(pl, batch, db, inflight, args.steps, ev, timing, local_rank)
    capi.sync()
    if dist is not None:
        _torch_sync()
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch
        tt = torch.tensor([elapsed], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        rr = torch.tensor([float(db.n_reads)], dtype=torch.float64, device=DIST_DEV)
        dist.all_reduce(rr, op=dist.ReduceOp.SUM)
        total_reads = float(rr.item())
    else:
        total_reads = float(db.n_reads)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res, pl)
    e2e_ranks = None
    if rank_bam is not None:
        # N ranks, N GPUs, ONE host: every rank types its own BAM file through hgx_type_file, all at the same time
        import shutil
        import torch
        try:
            hgx.type_file(pl, rank_bam)
            n_calls = 4
            _torch_sync()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(n_calls):
                r_f = hgx.type_file(pl, rank_bam)
            dt = time.perf_counter() - t0
            dist.barrier()
            tt = torch.tensor([dt], dtype=torch.float64, device=DIST_DEV)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ok = torch.tensor([1.0 if (r_f.gene_prob == res.gene_prob and r_f.num_reads == res.num_reads) else 0.0], dtype=torch.float64, device=DIST_DEV)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            e2e_ranks = {"input": "every rank its own coordinate-sorted BAM file, %d calls back to back, all ranks at once" % n_calls,
                         "ms_per_call": round(float(tt.item()) / n_calls * 1e3, 2),
                         "reads_per_s_all_ranks": round(total_reads * n_calls / float(tt.item()), 1),
                         "results_identical_to_hbm_path_on_every_rank": bool(ok.item() > 0.5),
                         "note": "hgx_type_file: the ranks share the node's host cores (cgroup quota: %s CPUs): this is where file -> result "
                                 "stops scaling with the GPUs" % cgroup_cpu_quota()}
        finally:
            shutil.rmtree(os.path.dirname(rank_bam), ignore_errors=True)

    # the same steps with SEVERAL samples in flight (host threads with their own streams, hgx_type_opts.gate): the reference's own unit of
    # scale is a pool of processes over samples (/root/reference/hisatgenotype:613-665); one sample's step is a chain of ~70 short
    # dependent launches that leaves most of the chip idle, the next sample's scoring fills it.  Reported beside `value`, never as it.
    in_flight = None
    if args.full and inflight == 1 and dist is None and not args.no_workloads and not args.no_in_flight:
        in_flight = {}
        for nf in (2, 3):
            n_st = 10 * nf
            run_steps(pl, batch, db, nf, 3 * nf, None, False, local_rank)           # (warm-up: the pool grows by the extra samples' buffers)
            capi.sync()
            t0 = time.perf_counter()
            run_steps(pl, batch, db, nf, n_st, None, False, local_rank)
            capi.sync()
            dt = time.perf_counter() - t0
            in_flight[str(nf)] = {"steps": n_st, "ms_per_step": round(dt / n_st * 1e3, 3), "value": round(db.n_reads * n_st / dt, 1)}
    # the same steps in the OTHER EM arithmetic, a few of them outside the timed region: `value` times the library's default (reference
    # order up to 4 096 classes, table lookups <= 1e-9 beyond: EM #1 of this sample); em_fast = -1 is the reference's order at every
    # size, bit-identical abundances (say what the bit-identical form costs NEXT to `value`)
    exact_em = None
    if args.full and inflight == 1 and dist is None and not args.no_workloads and not args.em_exact:
        EM_MODE = -1
        try:
            run_steps(pl, batch, db, 1, 1, None, False, local_rank)
            capi.sync()
            t0 = time.perf_counter()
            res_x, _, _, _ = run_steps(pl, batch, db, 1, 3, None, False, local_rank)
            capi.sync()
            dt = (time.perf_counter() - t0) / 3
            exact_em = {"ms_per_step": round(dt * 1e3, 3), "value": round(db.n_reads / dt, 1), "steps": 3,
                        "same_top2": [a for a, _ in res_x.gene_prob[:2]] == [a for a, _ in res.gene_prob[:2]],
                        "max_abs_abundance_difference_to_the_timed_form": max([abs(p - q) for (_, p), (_, q) in zip(res_x.gene_prob, res.gene_prob)] or [0.0])}
        except Exception as e:
            exact_em = {"error": repr(e)[:300]}
        finally:
            EM_MODE = False
    if rank == 0:
        # Per-kernel achieved rates from HIP events recorded inside the timed region (byte models: DESIGN.md section 5).
        #  k_lutmatvec<0> (EM rows pass): the compact class bit matrix once + its dense vectors
        #  k_pair_classes (the per-pair gene-level launch): the pairs' gene-level compat rows read + 1 class row (+ hash)
        #                  written per pair + refs/offsets
        #  k_piece_compat: n_words x a_pad x 4 index bytes read + one compat row written per distinct piece
        row = pl.a_pad // 8
        n_gene_refs = db.n_gene_refs
        # fused gene-level launch (hgx_pair_classes_dedup): the pairs' gene-level compat rows read, one representative row read
        # per pair for the exact compare (in place of the row + hash the unfused form wrote), refs / offsets, slot index written
        pc_bytes = n_gene_refs * row + 4 * db.n_refs + 4 * (db.n_pairs + 1) + db.n_pairs * (row + 4)
        cp_bytes = db.sum_piece_words * pl.a_pad * 4 + db.n_pieces * (row + 8) + db.sum_piece_words * 8
        pc_ms = sum(e[2].elapsed_ms(e[3]) for e in ev) / len(ev)
        cp_ms = sum(e[0].elapsed_ms(e[1]) for e in ev) / len(ev)
        gbs = lambda b, ms: (b / (ms * 1e-3) / 1e9) if ms > 0 else 0.0
        kernels = {}
        for name, (ms, n, ex, by) in em_timing.items():
            if n:
                # every plain rows / cols pass of the last N_TIMED_STEPS steps, timed with dispatch-attached events
                nts = min(N_TIMED_STEPS, args.steps)
                kernels[name] = {"timed_launches": n, "timed_steps": nts, "alg_bytes_per_launch": int(by // n),
                                 "avg_ms": round(ms / n, 5), "total_ms_per_step": round(ms / nts, 4), "GBps": round(gbs(by, ms), 1)}
        kernels["k_pair_classes"] = {"launches": args.steps, "alg_bytes_per_launch": int(pc_bytes), "avg_ms": round(pc_ms, 4),
                                     "total_ms_per_step": round(pc_ms, 4), "GBps": round(gbs(pc_bytes, pc_ms), 1)}
        # k_piece_compat_pat (round 4): the word tests are made once per DISTINCT value of a variant word, the per-allele work is
        # eight LDS reads per 64 pieces and a bit transpose; what has to cross the fabric is one compat row written per distinct
        # piece, the value-id tables of the window words read per group of 64 pieces (L2-resident: 1 B per allele and word at
        # HLA-A) and the piece table.  Priced against HBM (the rows are the kernel's only large stream); the kernel itself is
        # bound by the transposes' VALU issue and by launch width (996 groups of 64 pieces), not by bandwidth.
        n_groups = (db.n_pieces + 63) // 64
        cp_bytes = db.n_pieces * (row + 8) + db.sum_piece_words * 8 + n_groups * 8 * pl.a_pad
        kernels["k_piece_compat"] = {"launches": args.steps, "alg_bytes_per_launch": int(cp_bytes), "avg_ms": round(cp_ms, 4),
                                     "total_ms_per_step": round(cp_ms, 4), "GBps": round(gbs(cp_bytes, cp_ms), 1)}
        for k in kernels:
            if "bound" not in kernels[k]:
                kernels[k].update(bound="hbm", peak_GBps=HBM_PEAK_GBS, frac=round(kernels[k]["GBps"] / HBM_PEAK_GBS, 4))
        # largest aggregate time per step.  The EM's cols pass and the gene level's k_pair_classes are within a few per cent of each
        # other (0.50-0.54 ms per step each; the latter's HIP-event bracket also holds its wait for CUs beside the EM chain): among the
        # kernels within 5 % of the largest the one FURTHER from its roofline is reported, so that the figure does not flip between runs
        top = max(v["total_ms_per_step"] for v in kernels.values())
        dom = min((k for k in kernels if kernels[k]["total_ms_per_step"] >= 0.95 * top), key=lambda k: kernels[k]["frac"])
        alg_bytes, avg_ms = kernels[dom]["alg_bytes_per_launch"], kernels[dom]["avg_ms"]
        achieved = kernels[dom]["GBps"]
        traffic = None
        tf = os.path.join(ROOT, "profiles", "traffic.json")       # PMC passes of the same command (see profiles/README.md)
        if os.path.exists(tf):
            try:
                tj = json.load(open(tf))
                if tj.get("n_pairs") == db.n_pairs and tj.get("a_pad") == pl.a_pad:
                    traffic = tj["hbm_bytes_per_launch"].get(dom)
            except Exception:
                traffic = None
        # ---- the whole step against the roofline: algorithmic bytes of everything a step runs / its wall time ----
        # scoring: piece compat + the gene-level per-pair launch (above) + the exon level per DISTINCT ref list (rows read per ref, one
        # class row + hash written per group); dedup: every row hashed / inserted once and read once more by the exact verify, at both
        # levels; Gene_counts: the gene class matrix once; EM: every executed mat-vec pass streams its compact bit matrix + vectors
        n_exon_refs = db.n_refs - n_gene_refs
        try:
            n_exon_groups = engine.Groups(db, 0).n_groups
        except Exception:
            n_exon_groups = db.n_pairs
        exon_bytes = n_exon_refs * row // max(db.n_pairs // max(n_exon_groups, 1), 1) + n_exon_groups * (row + 12)
        dedup_bytes = 2 * db.n_pairs * (row + 8) + 2 * n_exon_groups * (row + 8)
        n_gene_cls = res.em[1]["n_classes"] if len(res.em) > 1 else 0
        em_bytes = sum(by / max(min(N_TIMED_STEPS, args.steps), 1) for (_ms, _n, _ex, by) in em_timing.values())
        step_alg_bytes = int(cp_bytes + pc_bytes + exon_bytes + dedup_bytes + em_bytes)
        ms_step = elapsed / args.steps * 1e3
        step_profile = None
        sp = os.path.join(ROOT, "profiles", "step_profile.json")   # tools/step_profile.py over the rocprofv3 kernel trace of this command
        if os.path.exists(sp):
            try:
                sj = json.load(open(sp))
                if sj.get("n_pairs") == db.n_pairs and sj.get("a_pad") == pl.a_pad:
                    step_profile = sj["per_step"]
                    step_profile["source"] = sj["source"]
            except Exception:
                step_profile = None
        cl_jobs, cl_fallbacks = engine.emx_cluster_stats()
        out = {
            "metric": "typed reads/sec at HLA-A (~7k alleles, 2x150bp)",
            "value": round(total_reads * args.steps / elapsed, 1),
            "unit": "reads/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64 bitsets, f64 EM",
            "data": "synthetic",
            "em_iters_per_s": round(n_em_iter / max(t_em, 1e-9), 1),
            "config": {
                "workload": "configs[1]: HLA-A-like locus, %d simulated 2x150bp reads per GPU, %d alleles, %d variants" % (
                    db.n_reads, pl.n_alleles, pl.n_vars),
                "pairs_per_gpu": db.n_pairs, "distinct_pieces": db.n_pieces, "piece_refs": db.n_refs,
                "exon_classes": res.em[0]["n_classes"] if res.em else 0,
                "gene_classes_after_handoff": res.em[1]["n_classes"] if len(res.em) > 1 else 0,
                "em_outer_iterations_per_step": n_em_iter // max(args.steps, 1),
                "em_arithmetic": "reference order at every size (hgx_type_opts.em_fast = -1: bit-identical abundances; EM #1 on one CU)" if args.em_exact
                                 else "default: reference order up to 4096 classes (EM #2 here), chip-wide table lookups beyond (EM #1 here, <= 1e-9)",
                "top2": [a for a, _ in res.gene_prob[:2]], "true_alleles": sample,
                "parallelism": "samples/loci shard over GPUs with no data-path collective; %d sample(s) in flight per GPU" % inflight,
                "comm_kind": comm_kind, "index_broadcast_bytes": bcast_bytes, "shared_gpu": bool(args.share_gpu),
                "input": "piece batch built in HBM by the device front end from the SAM text (route %d, decline code %d: %.1f ms, not timed; %s)" % (
                             fe_route, fe_code, t_parse_dev * 1e3,
                             "identical to the host front end's batch: %s -- the host takes %.1f ms on %d host threads" % (
                                 fe_same, t_parse * 1e3, os.cpu_count() or 1) if batch is not None else "compared with the host front end's batch under --full"),
                "device_front_end_batch_identical_to_host": bool(fe_same) if fe_same is not None else None,
                "setup_s": round(t_setup, 1),
            },
            "roofline": {
                "bound": "hbm", "kernel": dom,
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                "alg_bytes_per_launch": int(alg_bytes), "avg_launch_ms": round(avg_ms, 4),
                "note": "kernel with the largest aggregate time per step (of those within 5 % of the largest, the one further from its roofline); averages are over ALL its launches in the timed region "
                        "(incl. the tiny EM #2 problem and launches that exit at the convergence gate), as rocprofv3 --stats reports them",
                "kernels": kernels,
                # the step as a whole: how far from the machine, and where the rest goes
                "step_alg_bytes": step_alg_bytes,
                "step_frac": round(step_alg_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "step_alg_bytes_parts": {"piece_compat": int(cp_bytes), "pair_classes_gene": int(pc_bytes), "pair_classes_exon": int(exon_bytes),
                                         "dedup_both_levels": int(dedup_bytes), "em_passes": int(em_bytes)},
                "step_profile": step_profile,      # dispatches / kernel time / gaps per step, from the committed kernel trace of this command
                "emx_cluster_problems": cl_jobs, "emx_cluster_fallbacks": cl_fallbacks,
                "stream_sets": engine.stream_sets_info(),
            },
        }
        out["value_scope"] = ("`value`: rows 8a-5 ... 8a-9 of SURVEY.md section 8 (scoring, class dedup, Gene_counts, both EMs, hand-off, result) over a "
                              "piece batch resident in HBM, ONE sample at a time, the library's default EM arithmetic; rows 8a-1 ... 8a-4 (record decode, "
                              "filters, pileup, CIGAR x MD x Zs walk, haplotypes) are NOT in it -- `e2e` (file -> result) includes them")
        if exact_em:
            out["value_exact_em"] = exact_em.get("value")
            out["exact_em"] = exact_em
        if in_flight:
            out["value_3_in_flight"] = in_flight["3"]["value"]
            out["value_2_in_flight"] = in_flight["2"]["value"]
            out["samples_in_flight"] = {"note": "the timed steps again with 2 / 3 samples in flight on the GPU (one host thread and stream set per sample, the "
                                                "bandwidth-bound fronts taking turns); `value` above is ONE sample at a time", **in_flight}
        if pre is not None:
            out["e2e_scaling"] = pre[2]
        if e2e_ranks is not None:
            out["e2e"] = e2e_ranks
        if sam_keep is not None:
            if not args.no_e2e:
                out["e2e"] = end_to_end(pl, loc, sam_keep, res)
            cb, _ = cpu_baseline(loc, sam_keep, min(args.cpu_pairs, db.n_pairs))
            out["cpu_baseline"] = cb
            t_fe = (out.get("e2e") or {}).get("bam", {}).get("host_front_end_one_thread_s")
            if t_fe:
                t_cpu = t_fe + db.n_reads / cb["value"]
                out["e2e"]["cpu_baseline"] = {
                    "value": round(db.n_reads / t_cpu, 1), "unit": "reads/s", "cores": 1, "kind": "port",
                    "sample": "the same BAM file: host front end (read, inflate, walk, sort, decode; libhgx's C++ host stages, n_threads = 1) %.2f s "
                              "measured on the whole file + scoring / dedup / EM at the C oracle's rate (cpu_baseline: %.0f reads/s on its bounded "
                              "sample) = %.1f s for %d reads" % (t_fe, cb["value"], t_cpu, db.n_reads),
                    "gpu_over_cpu": {k: round((db.n_reads / (out["e2e"][k]["ms"] * 1e-3)) / (db.n_reads / t_cpu), 1) for k in ("sam", "bam")}}
    # ---- the other BASELINE.json workloads, driver-timed in the same run: configs[2] (class1) and configs[3] (panel64) --------
    if args.full and not args.no_workloads and (world == 1 or args.workloads):
        del batch, db
        import copy
        wl = {}
        for name, fn, steps, warm in (("class1", run_class1, args.wl_steps, 2), ("panel64", run_panel64, args.wl_steps, 2)):
            a2 = copy.copy(args)
            a2.steps, a2.warmup, a2.workload = steps, warm, name
            t0 = time.perf_counter()
            try:
                line = fn(a2, rank, local_rank, world, dist)
            except Exception as e:                                  # a side leg must not cost the run its headline ...
                if dist is not None:                                # (... but ranks that disagree about a failure would hang: re-raise)
                    raise
                line = {"error": repr(e)[:500]}
            if rank == 0:
                line["wall_s_incl_setup"] = round(time.perf_counter() - t0, 1)
                wl[name] = line
        if rank == 0 and world == 1:
            for wname, fixture in (("config0_dropin", "hla_7000_10k"), ("codis_dropin", "codis_10k"), ("sample6", None)):
                try:
                    wl[wname] = run_dropin(args, fixture) if fixture else run_sample6(args)
                except Exception as e:                              # (a side leg must not cost the run its headline)
                    wl[wname] = {"error": repr(e)[:500]}
        if rank == 0:
            out["workloads"] = wl
            c0 = wl.get("config0_dropin") or {}
            if "repeated_call_ms" in c0:
                # the one like-for-like comparison with the REAL reference there is: the same input, the same entry point
                out["reference_like_for_like"] = {
                    "input": "BASELINE configs[0]: tests/golden/hla_7000_10k (10 000 SAM records, 7 000 alleles), typing(<38 arguments>) -> report file",
                    "reference_seconds_recorded": c0["reference_recorded"]["seconds"], "reference_cpu": c0["reference_recorded"]["cpu"],
                    "this_first_call_ms": c0["first_call_ms"], "this_repeated_call_ms": c0["repeated_call_ms"],
                    "report_identical": c0["report_identical_to_the_reference"], "speedup": c0["speedup_over_the_recorded_reference"],
                    "note": "the reference was timed in the build container (one core, recorded with the fixture); this call on this box"}
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
