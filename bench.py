#!/usr/bin/env python3
"""bench.py -- headline benchmark of the block pipeline (dequantize -> IDCT -> YCbCr->RGB).

Contract (driver):  python bench.py --gpus N --steps K --warmup W
  N > 1: the driver launches  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N
  (one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the env).  Run plainly as
  `python bench.py --gpus N` (no WORLD_SIZE in the env) this script starts those N ranks itself, as
  fresh child processes, BEFORE anything touches the GPU, and relays rank 0's line.  In every case
  the line's n_gpus equals --gpus: a world size that differs from --gpus is an error (exit 2), never
  a silently smaller run.

Workload (BASELINE.json north_star / SURVEY 8d "roofline target"): a stream of synthetic
4096x4096 baseline 4:4:4 images, already Huffman-decoded into packed int16 coefficient blocks
resident in HBM.  One STEP = one pass of the hot path over one batch of IMAGES_PER_STEP such
images (one kernel launch; 4.8 GB of distinct input+output per step, so nothing is served from
the 256 MiB Infinity Cache).  Every rank owns its own batch (images shard by index, no
collective on the data path): weak scaling.

Prints ONE JSON line on rank 0:  metric = Mpixels/s decoded (whole job), ms_per_step = wall time of
one timed step (the K timed steps / K), plus
  roofline     achieved = algorithmic bytes per launch / mean kernel time (HIP events on the
               launch stream around sampled timed steps), against the 8 TB/s HBM3E peak;
               traffic = HBM bytes per launch from the committed PMC passes (profiles/), only
               when they were taken with THIS jb_kernels.hip (content hash), else null.
A plain run does only that: set up, pre-condition, warm up, time the K steps, print the line.

--dump-outputs DIR  after the timed steps, rank 0 writes what its last timed step handed back (the
               RGB images of that step's batch) as DIR/<name>.npy (dump_outputs(): exact per-row sums
               of all of it plus a fixed, seeded sample of its bytes).  The inputs are seeded, so two
               builds run with the same arguments can be compared output for output.

--full adds the measurements that take runs of their own (--no-configs / --no-e2e /
--no-cpu-baseline leave single ones out):
  configs      (N=1) the other single-GPU BASELINE.json configurations timed as stated: config 2
               = ONE 1920x1080 4:4:4 image per launch, config 3 = ONE 4096x4096 4:2:0 image per
               launch, both COLD (rotating buffer sets totalling > 512 MiB, twice the Infinity
               Cache), HIP events around every launch, median of >= 200; plus the per-GPU shares
               of the batch configs and the reference's bundled-image size;
  end_to_end   decode(path) over batches of synthetic JPEG FILES (written by the build's own baseline
               writer): BASELINE.json configs 4 and 5 in two forms -- weak: every rank decodes one
               GPU's share at 8 GPUs (128 x 1920x1080 4:4:4, 32 x 8192x8192 4:2:0); strong: the
               batch as stated (1,024 / 256 files) dealt over the ranks by image index --
               through jb_batch_decoder: parse + byte de-stuffing on the host threads, Huffman
               decoding + IDCT + colour on the device, pixels into pinned host memory (PCIe-
               inclusive, so never `value`); images/s = all ranks' images / the slowest rank's wall;
               at N=1 also with the entropy stage on the host threads (north_star's split); and
               with the decoded images left in device memory (jb_batch_decoder_set_device_output);
  cpu_baseline the reference CPU path (oracle/_ref, the genuine reference compiled in place,
               kind "reference") or, if that build is absent, the C restatement (kind "port"),
               timed on this box's host cores on a bounded sample -- rank 0, N=1 only.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMAGES_PER_STEP = 32  # 4.8 GB per launch: the drain of one launch is 1/4 of what it is with 8 images (+2 % kernel rate)
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
SAMPLING = {"444": (1, 1), "420": (2, 2), "422": (2, 1), "440": (1, 2)}
SAMPLING_NAME = {(1, 1): "4:4:4", (2, 2): "4:2:0", (2, 1): "4:2:2", (1, 2): "4:4:0"}
KERNEL_SOURCE = os.path.join(ROOT, "jpeg_decoder_amd", "csrc", "jb_kernels.hip")

# (key, workload, images per launch, rotating buffer sets, what it is) -- BASELINE.json configs 2-5
# on one GPU.  A "cold" entry cycles through enough distinct buffer sets (> 512 MiB in total) that
# no launch finds its input or output in the 256 MiB Infinity Cache.
EXTRA_CONFIGS = [
    ("config2_single_1080p_444_cold", "1920x1080-444", 1, 32, "BASELINE config 2: ONE 1920x1080 4:4:4 image per launch, cold"),
    ("config3_single_4096_420_cold", "4096x4096-420", 1, 8, "BASELINE config 3: ONE 4096x4096 4:2:0 image per launch, cold"),
    ("config3_stream_4096_420_x8", "4096x4096-420", 8, 1, "config 3 shape as a stream: 8 images per launch"),
    ("config4_share_1080p_444_x128", "1920x1080-444", 128, 1, "BASELINE config 4, one GPU's share: 128 x 1920x1080 4:4:4 in one launch"),
    ("config5_share_8192_420_x4", "8192x8192-420", 4, 1, "BASELINE config 5 shape: 4 x 8192x8192 4:2:0 in one launch"),
    ("bundled_size_679x451_420_x512", "679x451-420", 512, 1, "the reference's bundled images/img.jpg size, 512 per launch, tightly packed odd-width rows"),
    ("bundled_size_679x451_420_x512_pitch2048", "679x451-420@2048", 512, 1, "the same 512 images with a row pitch of 2048 bytes (the next multiple of 64 above 3*679 = 2037): what a caller that chooses its pitch gets"),
]


def parse_workload(text):
    text = text.split("@")[0]   # ("WxH-SSS@P": row pitch P bytes, Resident reads it)
    dims, samp = text.split("-")
    w, h = (int(v) for v in dims.split("x"))
    hs, vs = SAMPLING[samp]
    return w, h, hs, vs


def kernel_source_hash():
    with open(KERNEL_SOURCE, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def cpu_baseline(width, height, hs, vs, coef, qtabs, budget_s=12.0):
    """Reference CPU path on one host core (the reference is single-threaded), bounded sample."""
    from oracle.pyoracle import Oracle, Ref, make_desc
    desc = make_desc(width, height, hs, vs)
    mpix = width * height / 1e6
    out = {}
    ref_present = Ref.available()
    if ref_present:
        ref = Ref()
        ms = [0.0, 0.0, 0.0]
        t_hot, reps, t0 = 0.0, 0, time.time()
        while time.time() - t0 < budget_s:
            ref.blocks_to_rgb(desc, coef, qtabs, stage_ms=ms)
            t_hot += sum(ms) / 1e3
            reps += 1
        out = {"value": round(mpix * reps / t_hot, 2), "unit": "Mpixels/s", "cores": 1, "kind": "reference",
               "sample": f"{reps} x one {width}x{height} {SAMPLING_NAME[(hs, vs)]} image through the reference's own "
                         f"dequantize+inverseDCT+YCbCrToRGB (oracle/_ref, g++ -O2), {t_hot:.1f} s"}
    ora = Oracle()
    reps = 3
    s1 = ora.time_blocks_to_rgb(desc, coef, qtabs, 1, reps)
    port1 = mpix * reps / s1
    ncores = os.cpu_count() or 1
    nthr = min(ncores, 64)
    reps_mt = 8
    smt = ora.time_blocks_to_rgb(desc, coef, qtabs, nthr, reps_mt)
    if not out:
        out = {"value": round(port1, 2), "unit": "Mpixels/s", "cores": 1, "kind": "port",
               "sample": f"{reps} x one {width}x{height} {SAMPLING_NAME[(hs, vs)]} image through oracle/jpegblk_oracle.c (gcc -O2), {s1:.1f} s"}
    try:
        model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except Exception:
        model = "unknown"
    # the genuine-reference build (oracle/_ref) is git-ignored and only exists where it was built
    # from /root/reference: say whether THIS run had it, so a "port" line cannot pass for a "reference" one
    out["ref_present"] = bool(ref_present)
    out["cpu_model"] = model
    out["flags"] = "reference harness: g++ -O2 -fno-access-control -U_FORTIFY_SOURCE (oracle/Makefile); port: gcc -O2 -ffp-contract=off; no -march=native, no -ffast-math"
    out["port_1core_mpix_s"] = round(port1, 2)
    out["port_allcores_mpix_s"] = round(mpix * reps_mt / smt, 2)
    out["port_allcores_threads"] = nthr
    out["host_cpus"] = ncores
    return out


DUMP_BUDGET_BYTES = 64 << 20   # --dump-outputs writes at most this much in all
DUMP_SAMPLE_BYTES = 1 << 23    # image bytes in the seeded sample (32 MB as float32)
DUMP_SEED = 20240611


def dump_outputs(out_dir, np, torch, res, rgb_t):
    """--dump-outputs: the images one step of the timed path handed back, rgb_t = uint8 [images, h, pitch]
    on the device (pixel row y of image i = rgb_t[i, y, :3w]), as float arrays:
      rgb_row_sums.npy  float64 [images, h]  the sum of every pixel row's 3w bytes (exact): all of the output
      rgb_sample.npy    float32 [n]          the bytes at n positions drawn with a fixed seed from the
                                             images' pixel bytes (row-major over [images, h, 3w], ascending)
    n = min(DUMP_SAMPLE_BYTES, all pixel bytes), less if the row sums would push the total over
    DUMP_BUDGET_BYTES; the positions depend only on the workload, so equal arguments give equal files."""
    os.makedirs(out_dir, exist_ok=True)
    row = 3 * res.w
    pix = rgb_t[:, :, :row]
    sums = pix.sum(dim=2, dtype=torch.int64).cpu().numpy().astype(np.float64)
    np.save(os.path.join(out_dir, "rgb_row_sums.npy"), sums)
    total = res.nimg * res.h * row
    n = max(0, min(DUMP_SAMPLE_BYTES, total, (DUMP_BUDGET_BYTES - sums.nbytes) // 4))
    pos = np.sort(np.random.default_rng(DUMP_SEED).integers(0, total, size=n, dtype=np.int64))
    img, rest = np.divmod(pos, res.h * row)
    y, x = np.divmod(rest, row)
    off = torch.from_numpy(img * (res.h * res.pitch) + y * res.pitch + x).to(rgb_t.device)
    sample = rgb_t.reshape(-1)[off].to(torch.float32).cpu().numpy()
    np.save(os.path.join(out_dir, "rgb_sample.npy"), sample)


def fan_out(n_gpus, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes
    (torch.distributed.run, one per GPU).  Called before this process has imported torch or made
    any HIP call, so no process that touched the GPU is ever replaced or forked."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, JB_BENCH_FANNED_OUT="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


# (key, workload, files in the whole batch as BASELINE.json states it, files per GPU when weak-scaled = the share at 8 GPUs,
#  distinct files, restart interval in MCU rows, what it is)
E2E_CONFIGS = [
    ("config4_files_1080p_444", "1920x1080-444", 1024, 128, 8, 0, "BASELINE config 4: 1024 x 1920x1080 4:4:4 JPEG files"),
    ("config5_files_8192_420", "8192x8192-420", 256, 32, 4, 0, "BASELINE config 5: 256 x 8192x8192 4:2:0 JPEG files"),
]
E2E_SUB_BATCH_BYTES = 8 << 30   # a rank's share is decoded in sub-batches whose pixels fit a pinned arena of this size


def host_threads(world):
    """Host threads of one rank: device-entropy batches need few (they parse, de-stuff and pack: 16 saturate the
    link), host-entropy batches take every CPU the rank may use (the library clamps by the cgroup quota as well)."""
    cpus = max(1, len(os.sched_getaffinity(0)) // world)
    return max(2, min(16, cpus)), max(2, min(64, cpus))


def end_to_end(jb, np, torch, dist, dev_index, reduce_device, rank, world, tmpdir):
    """decode(path) over batches of files; -> dict (identical on all ranks).  Two forms per configuration:
    weak   every rank decodes one GPU's share at 8 GPUs (128 / 32 files): the per-GPU rate as N grows;
    strong the batch BASELINE.json states (1,024 / 256 files) is dealt over the ranks by image index
           (jpeg_decoder_amd.shard.shard_images): at N = 8 both forms are the same batch."""
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.shard import job_throughput, shard_images
    thr_dev, thr_host = host_threads(world)
    out = {"what": "jb_batch_decoder over JPEG files on local disk (page cache): parse + de-stuffing on the host threads, "
                   "entropy decoding + IDCT + colour on the device, pixels into a pinned host arena; images/s = all ranks' images / the slowest rank's wall",
           "host_cpus": os.cpu_count(), "cpu_affinity": len(os.sched_getaffinity(0)),
           "host_threads_per_gpu": {"entropy_on_device": thr_dev, "entropy_on_host": thr_host},
           "files": "synthetic blocks through tools/jpegwriter (Annex-K Huffman tables, quality-75 quantisation), distinct per size as listed, the rest repeats",
           "checked_against": "the single-image decode(path) with the entropy stage on the HOST decoder (JPEGBLK_GPU_HUFFMAN=0), "
                              "itself pinned to the reference's coefficient dumps and the oracle by tests/: one image of every distinct file per rank and form",
           "runs": {}}
    for key, wl, total, per_gpu, distinct, ri_rows, what in E2E_CONFIGS:
        w, h, hs, vs = parse_workload(wl)
        coef, q = synth.synth_blocks(w, h, hs, vs, image_index=7)
        bpm = hs * vs + 2
        mcus_x = (w + 8 * hs - 1) // (8 * hs)
        paths = []
        for i in range(distinct):
            path = os.path.join(tmpdir, f"{key}_{i}.jpg")
            with open(path, "wb") as f:
                f.write(synth.encode_jpeg(np.roll(coef, i * 4099 * bpm, axis=0), w, h, hs, vs, q, restart_interval=ri_rows * mcus_x))
            paths.append(path)
        del coef
        os.environ["JPEGBLK_GPU_HUFFMAN"] = "0"
        with jb.Context(dev_index) as one:
            want = [one.decode_file(p) for p in paths]
        os.environ.pop("JPEGBLK_GPU_HUFFMAN", None)
        g = jb.geometry_of(jb.make_desc(w, h, hs, vs))
        per = (g.rgb_bytes + 255) // 256 * 256
        res = {"what": what, "workload": wl, "batch_files": total, "files_per_gpu_weak": per_gpu, "distinct_files": distinct,
               "file_bytes": os.path.getsize(paths[0])}
        forms = [("weak", list(range(per_gpu)))]
        mine = shard_images(total, rank, world)
        forms.append(("strong", mine))
        for form, idx in forms:
            files = [paths[i % distinct] for i in idx]
            n_mine = len(files)
            sub = max(1, min(n_mine, E2E_SUB_BATCH_BYTES // per))   # files per run (one arena's worth)
            fres = {"files_this_rank": n_mine, "files_per_run": sub, "runs": (n_mine + sub - 1) // sub,
                    "runs_overlap": "two in flight (jb_batch_decoder_submit / _collect)" if n_mine > sub else "one run"}
            modes = [("device", None, thr_dev)] + ([("host", "0", thr_host)] if world == 1 else [])
            for label, knob, threads in modes:
                if knob is None:
                    os.environ.pop("JPEGBLK_GPU_HUFFMAN", None)
                else:
                    os.environ["JPEGBLK_GPU_HUFFMAN"] = knob
                bad, seen = [], set()

                def check(i, view, base=0):
                    k = idx[base + i] % distinct
                    if k not in seen:
                        seen.add(k)
                        if not np.array_equal(view, want[k]):
                            bad.append(base + i)

                with jb.BatchDecoder(threads, dev_index, g.coef_bytes, g.rgb_bytes, arena_bytes=sub * per) as dec:
                    dec.run(files[:min(threads, sub)], keep_pixels=False)
                    walls = []
                    # pass 0 is the checked one and is not timed (it is also the decoder's first run); then the timed passes
                    reps = 3 if n_mine * per <= (16 << 30) else 2
                    runs = [(at, files[at:at + sub]) for at in range(0, n_mine, sub)]

                    def settle(st, key=key, form=form):
                        if any(x != 0 for x in st) or bad:
                            raise RuntimeError(f"end_to_end {key} {form}: statuses {sorted(set(st))}, images that differ from the host-entropy decode: {bad}")

                    for k in range(reps + 1):
                        if dist is not None:
                            dist.barrier()
                        if len(runs) == 1:
                            _, st, tm = dec.run(runs[0][1], keep_pixels=False, on_image=(lambda i, v: check(i, v, 0)) if k == 0 else None)
                            settle(st)
                            wall = tm["wall_s"]
                        else:
                            # a share larger than one arena: its sub-batches as a stream, two in flight (jb_batch_decoder_submit /
                            # _collect: each side has an arena; the start-up of one sub-batch runs under the tail of the one before)
                            t0 = time.perf_counter()
                            flight = []
                            for at, fl in runs + [(None, None), (None, None)]:
                                if fl is not None:
                                    flight.append((dec.submit(fl), at))
                                if len(flight) == 2 or (fl is None and flight):
                                    tk, base = flight.pop(0)
                                    _, st, tm = dec.collect(tk, keep_pixels=False, on_image=(lambda i, v, base=base: check(i, v, base)) if k == 0 else None)
                                    settle(st)
                            wall = time.perf_counter() - t0
                        n_all, wall = job_throughput(dist, reduce_device, n_mine, wall)
                        if k > 0:
                            walls.append(wall)
                    on_device = dec.device_entropy_images > 0
                best, med = min(walls), sorted(walls)[len(walls) // 2]
                fres[f"entropy_on_{label}"] = {"images_per_s": round(n_all / best, 1), "images_per_s_median": round(n_all / med, 1),
                                               "mpix_s": round(n_all * w * h / best / 1e6, 1), "wall_s": round(best, 4),
                                               "walls": [round(x, 4) for x in walls], "images": int(n_all), "host_threads": threads,
                                               "entropy_stage_ran_on_device": bool(on_device), "distinct_files_checked_per_rank": len(seen)}
            os.environ.pop("JPEGBLK_GPU_HUFFMAN", None)
            if form == "weak":
                # the same share with the decoded images left in device memory (jb_batch_decoder_set_device_output):
                # nothing is downloaded, so this is what the pipeline does when the link is not in the way
                region = torch.empty(n_mine * per, dtype=torch.uint8, device=f"cuda:{dev_index}")
                with jb.BatchDecoder(thr_dev, dev_index, g.coef_bytes, g.rgb_bytes) as dec:
                    dec.set_device_output(region.data_ptr(), region.numel())
                    dec.run_to_device(files[:thr_dev])
                    walls = []
                    for k in range(6):   # pass 0 is the checked one and is not timed, as above
                        if dist is not None:
                            dist.barrier()
                        ptrs, dims, st, tm = dec.run_to_device(files)
                        if any(x != 0 for x in st):
                            raise RuntimeError(f"end_to_end {key} (device output): statuses {sorted(set(st))}")
                        if k == 0:
                            for i in range(min(distinct, n_mine)):
                                off = ptrs[i] - region.data_ptr()
                                if not np.array_equal(region[off:off + g.rgb_bytes].cpu().numpy().reshape(want[0].shape), want[idx[i] % distinct]):
                                    raise RuntimeError(f"end_to_end {key} (device output): image {i} differs from the host-entropy decode")
                        n_all, wall = job_throughput(dist, reduce_device, n_mine, tm["wall_s"])
                        if k > 0:
                            walls.append(wall)
                best, med = min(walls), sorted(walls)[len(walls) // 2]
                fres["entropy_on_device_pixels_stay_in_hbm"] = {"images_per_s": round(n_all / best, 1), "images_per_s_median": round(n_all / med, 1),
                                                                "mpix_s": round(n_all * w * h / best / 1e6, 1), "wall_s": round(best, 4),
                                                                "walls": [round(x, 4) for x in walls], "images": int(n_all),
                                                                "distinct_files_checked_per_rank": min(distinct, n_mine)}
                del region
                torch.cuda.empty_cache()
            res[form] = fres
        out["runs"][key] = res
        for p_ in paths:
            os.remove(p_)
    return out


class Resident:
    """`sets` buffer sets of `nimg` images each, resident in HBM, plus the launch descriptors."""

    def __init__(self, jb, torch, dev, workload, nimg, sets, seed):
        from jpeg_decoder_amd import synth
        from jpeg_decoder_amd.api import torch_batch
        self.w, self.h, self.hs, self.vs = parse_workload(workload)
        self.pitch = int(workload.split("@")[1]) if "@" in workload else 3 * self.w   # bytes per pixel row in HBM
        self.nimg, self.sets = nimg, sets
        self.desc = jb.make_desc(self.w, self.h, self.hs, self.vs)
        g = self.g = jb.geometry_of(self.desc)
        # one seeded image on the host; every other image is an MCU-rotation of it made on the
        # device (distinct bytes, same statistics)
        self.coef, self.qtabs = synth.synth_blocks(self.w, self.h, self.hs, self.vs, image_index=seed)
        base = torch.from_numpy(self.coef).to(dev)
        self.q_t = torch.from_numpy(jb.resolve_qtabs(self.desc, self.qtabs)).to(dev)
        self.tensors, self.batches = [], []
        for s in range(sets):
            coef_t = torch.empty((nimg, g.n_coded_blocks, 64), dtype=torch.int16, device=dev)
            for i in range(nimg):
                coef_t[i] = torch.roll(base, shifts=((s * nimg + i) * 7919 % max(1, g.mcus_x * g.mcus_y)) * g.blocks_per_mcu, dims=0)
            rgb_t = torch.zeros((nimg, self.h, self.pitch), dtype=torch.uint8, device=dev)
            self.tensors.append((coef_t, rgb_t))
            self.batches.append(torch_batch(self.desc, nimg, coef_t, self.q_t, rgb_t))
        del base
        self.alg_bytes = nimg * (g.n_coded_blocks * 128 + self.w * self.h * 3)  # 128 B/block in + 3 B/pixel out
        self.pixels = nimg * self.w * self.h
        self.kernel = jb.lib().jb_kernel_name(self.desc).decode()
        # launches of up to 8 workgroups per CU take the one-wave kernels (csrc/jb_api.cpp
        # kSmallGridBelowPerCu; JPEGBLK_SMALL_GRID forces either)
        per_tile = {(1, 1): 64, (2, 2): 32, (2, 1): 64, (1, 2): 64}.get((self.hs, self.vs))
        knob = os.environ.get("JPEGBLK_SMALL_GRID", "")[:1]
        if per_tile:
            tiles = nimg * ((g.mcus_x * g.mcus_y + per_tile - 1) // per_tile)
            if knob == "1" or (knob != "0" and tiles <= 8 * torch.cuda.get_device_properties(dev).multi_processor_count):
                self.kernel = {(1, 1): "jb_small_kernel_444", (2, 2): "jb_small_kernel_420", (2, 1): "jb_small_kernel_16<2, 1>",
                               (1, 2): "jb_small_kernel_16<1, 2>"}[(self.hs, self.vs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precondition", type=int, default=400,
                    help="untimed launches before the warm-up steps (lets clocks/power settle)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run configs (N=1), end_to_end and cpu_baseline (N=1); "
                         "a plain run measures the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (rank 0; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the extra per-config measurements (N=1)")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the decode(path) batches over JPEG files (configs 4 and 5 end to end)")
    ap.add_argument("--images-per-step", type=int, default=IMAGES_PER_STEP)
    ap.add_argument("--sets", type=int, default=1, help="rotating buffer sets (cold single-image runs: > 512 MiB in total)")
    ap.add_argument("--workload", default="4096x4096-444",
                    help="WxH-444|420|422|440 (default = the headline workload; the others are what the "
                         "`configs` entries and the A/B tools run)")
    args = ap.parse_args()
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        sys.exit(2)
    launched = "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not launched:
        sys.exit(fan_out(args.gpus, sys.argv[1:]))
    from jpeg_decoder_amd.shard import rank_from_env
    # rehearsal knob (never set by the driver): every rank on device 0 of a one-GPU box
    single_device = os.environ.get("JB_BENCH_SINGLE_DEVICE") == "1"
    world, rank, local_rank = rank_from_env(os.environ, single_device)
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a {world}-rank run as {args.gpus} GPUs "
              f"(launch with --nproc-per-node {args.gpus}, or run `python bench.py --gpus {args.gpus}` without a launcher)",
              file=sys.stderr)
        sys.exit(2)
    WIDTH, HEIGHT, HS, VS = parse_workload(args.workload)

    import numpy as np
    import torch
    import jpeg_decoder_amd as jb

    dist = None
    # rehearsal knobs (never set by the driver): run N ranks on a one-GPU box
    backend = os.environ.get("JB_BENCH_BACKEND", "nccl")  # "nccl" = RCCL on ROCm
    if jb.lib().jb_device_count() < 1:
        raise RuntimeError("bench.py needs a HIP device: " + jb.lib().jb_last_error(None).decode())
    if not single_device and jb.lib().jb_device_count() < world:
        print(f"bench.py: {world} ranks but only {jb.lib().jb_device_count()} HIP devices visible", file=sys.stderr)
        sys.exit(2)
    if world > 1 or os.environ.get("JB_BENCH_FORCE_DIST") == "1":  # the latter: rehearse the RCCL path with one rank
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(backend)
    n_gpus = world
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")

    # all device work of this benchmark runs on one explicit torch stream, and the kernel is
    # launched on that same stream through the C ABI, so torch.cuda.Event times the kernel
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = jb.Context(local_rank)

    def barrier():
        if dist is not None:
            dist.barrier()

    def run(res, steps, warmup, precondition, every):
        """precondition + warmup untimed launches, then `steps` timed ones (barrier + sync on both
        sides); HIP events on the launch stream bracket every `every`-th timed launch."""
        nb = len(res.batches)
        k_launch = 0

        def step():
            nonlocal k_launch
            ctx.blocks_to_rgb_device(res.batches[k_launch % nb], stream.cuda_stream)
            k_launch += 1

        for _ in range(precondition):
            step()
        torch.cuda.synchronize()
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(0, steps, every)]
        t0 = time.perf_counter()
        for k in range(steps):
            if k % every == 0:
                evs[k // every][0].record(stream)
            step()
            if k % every == 0:
                evs[k // every][1].record(stream)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        return elapsed, [a.elapsed_time(b) for a, b in evs]

    # ---- headline ----
    # Pre-conditioning (untimed, before the W warm-up steps): MI355X power management needs a
    # few hundred back-to-back launches of this kernel to settle (launch times go 240 -> 350 ->
    # 240 us over the first ~100 launches, tools/steps.py); a stream workload runs in the settled
    # state, so that is the state the K timed steps are taken in.
    # HIP events bracket a sample of the timed steps (at least ~20 of them, every step when K is
    # small).  Event packets between back-to-back launches are measurement overhead that the
    # whole-job clock sees: with a pair around EVERY one of 200 steps ms_per_step was 3.7 % higher
    # (0.2110 vs 0.2035 ms) while the bracketed kernel time was the same (JB_BENCH_EVENT_EVERY overrides)
    every = max(1, int(os.environ.get("JB_BENCH_EVENT_EVERY", str(max(1, args.steps // 25)))))
    nimg = args.images_per_step
    head = Resident(jb, torch, dev, args.workload, nimg, args.sets, seed=rank)
    elapsed, kern_ms = run(head, args.steps, args.warmup, args.precondition, every)
    if args.dump_outputs and rank == 0:
        # the last timed launch wrote buffer set (launches - 1) % sets
        last = (args.precondition + args.warmup + args.steps - 1) % head.sets
        dump_outputs(args.dump_outputs, np, torch, head, head.tensors[last][1])
    from jpeg_decoder_amd.shard import job_throughput
    total_pixels, elapsed = job_throughput(dist, dev if backend == "nccl" else torch.device("cpu"),
                                           head.pixels * args.steps, elapsed)
    alg_bytes = head.alg_bytes
    mean_ms = float(np.mean(kern_ms))
    achieved = alg_bytes / (mean_ms * 1e-3) / 1e9
    value = total_pixels / elapsed / 1e6
    head_coef, head_q, head_kernel = head.coef, head.qtabs, head.kernel
    del head
    torch.cuda.empty_cache()

    e2e = None
    if args.full and not args.no_e2e:
        import tempfile
        with tempfile.TemporaryDirectory(dir="/tmp") as tmpdir:
            e2e = end_to_end(jb, np, torch, dist, local_rank, dev if backend == "nccl" else torch.device("cpu"), rank, world, tmpdir)

    if rank == 0:
        traffic, traffic_note = None, "no profiles/pmc_latest.json"
        pmc = os.path.join(ROOT, "profiles", "pmc_latest.json")
        if os.path.exists(pmc):
            try:
                rec = json.load(open(pmc))
                # the PMC passes profile the default command with ONE state of the kernel source:
                # only report them for that workload and that source
                if rec.get("algorithmic_bytes_per_launch") != alg_bytes:
                    traffic_note = "pmc_latest.json is for another workload"
                elif rec.get("kernel_source_sha256_16") != kernel_source_hash():
                    traffic_note = f"pmc_latest.json ({rec.get('tag')}) was taken with another jb_kernels.hip: stale, not reported"
                else:
                    traffic, traffic_note = rec.get("hbm_bytes_per_launch"), f"profiles/{rec.get('tag')}: FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes"
            except Exception as e:  # noqa: BLE001
                traffic_note = f"pmc_latest.json unreadable: {e}"
        line = {
            "metric": "Mpixels/s decoded (IDCT+colour)", "value": round(value, 1), "unit": "Mpixels/s",
            "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "precondition": args.precondition,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"stream of {WIDTH}x{HEIGHT} baseline {SAMPLING_NAME[(HS, VS)]} images, {nimg} images per step "
                                   f"(one launch) per GPU, coefficient blocks resident in HBM",
                       "images_per_step_per_gpu": nimg, "sampling": SAMPLING_NAME[(HS, VS)], "parallelism": f"images sharded x{n_gpus}, no collective",
                       "launched_by": "bench.py" if (not launched or os.environ.get("JB_BENCH_FANNED_OUT") == "1") else "torch.distributed.run"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_source": traffic_note,
                         "kernel": head_kernel, "kernel_source_sha256_16": kernel_source_hash(), "algorithmic_bytes_per_launch": alg_bytes,
                         "kernel_samples": len(kern_ms), "event_every": every,
                         "kernel_ms_mean": round(mean_ms, 4), "kernel_ms_median": round(float(np.median(kern_ms)), 4), "kernel_ms_min": round(float(np.min(kern_ms)), 4),
                         "kernel_gpix_s": round(nimg * WIDTH * HEIGHT / (mean_ms * 1e-3) / 1e9, 2)},
        }
        if args.full and n_gpus == 1 and not args.no_configs:
            # the other single-GPU configurations of BASELINE.json, timed as stated (events around
            # every launch, median of >= 200 launches; cold entries rotate over > 512 MiB of buffers)
            cfgs = {}
            for key, wl, n, sets, what in EXTRA_CONFIGS:
                res = Resident(jb, torch, dev, wl, n, sets, seed=1)
                launches = 400 if n == 1 else 200
                _, ms = run(res, launches, 20, 100, 1)
                med, mn = float(np.median(ms)), float(np.mean(ms))
                ach = res.alg_bytes / (med * 1e-3) / 1e9
                cfgs[key] = {"what": what, "workload": wl, "images_per_launch": n, "buffer_sets": sets,
                             "distinct_bytes": sets * res.alg_bytes, "cold": sets * res.alg_bytes > (512 << 20),
                             "launches": launches, "kernel": res.kernel,
                             "kernel_us_median": round(med * 1e3, 2), "kernel_us_mean": round(mn * 1e3, 2), "kernel_us_min": round(float(np.min(ms)) * 1e3, 2),
                             "algorithmic_bytes_per_launch": res.alg_bytes, "achieved": round(ach, 1), "unit": "GB/s",
                             "frac": round(ach / HBM_PEAK_GBPS, 4), "mpix_s": round(res.pixels / (med * 1e-3) / 1e6, 1)}
                del res
                torch.cuda.empty_cache()
            line["configs"] = cfgs
        if e2e is not None:
            line["end_to_end"] = e2e
        if args.full and n_gpus == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(WIDTH, HEIGHT, HS, VS, head_coef, head_q)
        print(json.dumps(line), flush=True)
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
