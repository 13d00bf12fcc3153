#!/usr/bin/env python3
"""Benchmark of the AlignSDF reconstruction hot path on MI355X.

A "step" is one sample through the path BASELINE.json names: bind latent (K0 fold) -> dense-grid SDF decode of
both heads on [-1,1]^3 (K1, with the negative-voxel bbox fused) -> zoom cube -> second N^3 decode (K1) ->
Lewiner marching cubes on the hand and the object volume (K3-K6).  Weights and codes are resident in HBM
before the timed region; the meshes stay on the device.  One step yields 2 meshes (hand + object).  The K timed
steps run through the product's own sample pipeline (alignsdf_amd.reconstruct.pipelined_two_pass), started empty
and drained inside the timed region.

Round 6: `value` / `ms_per_step` / `dtype` / the top-level `roofline` describe the product's DEFAULT, which is
the reference's arithmetic class on EVERY voxel of both lattices (networks/model.py:285-350 evaluates every point in fp32): ordinary
sweeps on the split-half kernel - 22-bit operands, fp32 accumulate, <= 1e-5 (measured 5.4e-7 against the fp32 chain on all 33.5 M
voxels).  The opt-in `--fast` sweeps (one fp16 plane for the SIGNS of a pass with one consumer + exact values wherever a value is
read + a statistical certificate: DESIGN.md 3c) are a secondary leg: `config.meshes_per_s_audited_sign_sweeps`.

    python bench.py --gpus N --steps K --warmup W [--grid 256] [--tag nerf3|both9] [--fast] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line; `--dump-outputs DIR` then also writes the arrays the last timed
step handed its caller (meshes and zoom cube, `DIR/<name>.npy`).  Everything else - the other kind of sweeps, the fp32 MFMA chain, the
sustained leg, the marching-cubes roofline, the other configurations, the CPU baseline, the comparisons with the reference's runs and
the side file of the whole record - runs only under `--full`.

Multi-GPU: samples are independent, so ranks share nothing on the data path (weak scaling: K samples per GPU); the
per-sample records are gathered to rank 0 over RCCL at the end.  One process per GPU.  Either the caller launches the
ranks (torch.distributed.run: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), or - when `--gpus N` is given
with N > 1 and no WORLD_SIZE is set - this script spawns the N ranks itself (one child process per GPU, rendezvous on
127.0.0.1) and relays rank 0's line.  `n_gpus` in the line is the value of an all_reduce of ones over the process group,
i.e. the number of ranks that actually took part.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_POINT_HEAD = 1_573_888      # dense formulation the reference executes
EXEC_FLOP_PER_POINT_HEAD = 2 * (4 * 512 + 512 * 256 + 260 * 512 + 512 * 512 + 512)   # after folding the latent columns
PEAK_FP32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2516.6        # MI355X_MICROARCH.md: dense BF16/F16 MFMA (v_mfma_f32_32x32x16_f16: 32 cycles/SIMD at 2.4 GHz)
PEAK_HBM_GBS = 8000.0                # MI355X_MICROARCH.md: HBM3E spec peak
# split-half kernel: the three hidden GEMMs issue 3 fp16 MFMAs per product sum (padded shapes), layers 0 / 2's point
# features stay on the fp32 MFMA
EXEC_F16_FLOP_PER_POINT_HEAD = 3 * 2 * (512 * 256 + 256 * 512 + 512 * 512)
EXEC_F16_SIDE_F32_FLOP_PER_POINT_HEAD = 2 * (4 * 512 + 4 * 512 + 512)
# one-plane kernel: ONE fp16 MFMA per product sum of the hidden GEMMs, + layer 0's point features and bias row as one K = 16 fp16
# MFMA per output tile; layer 2's point features stay on the fp32 MFMA
EXEC_P1_FLOP_PER_POINT_HEAD = 2 * (512 * 256 + 256 * 512 + 512 * 512) + 2 * 16 * 512
EXEC_P1_SIDE_F32_FLOP_PER_POINT_HEAD = 2 * (4 * 512 + 512)
CHUNK = 2 ** 18                      # reconstruct.py:93


# ------------------------------------------------------------------------------------------------------------------
# launching: --gpus N without an external launcher
# ------------------------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_environments(n, base_env=None, port=None):
    """Environment of each of the n ranks this script spawns (what torch.distributed.run would export)."""
    port = port or free_port()
    envs = []
    for r in range(n):
        e = dict(base_env if base_env is not None else os.environ)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port))
        e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # the host driver only supports dmabuf IPC (RCCL needs it)
        envs.append(e)
    return envs


def spawn_ranks(n, argv, timeout=None):
    """Run this script once per rank; relay rank 0's stdout (the JSON line).  Returns the exit code."""
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=e, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL)
             for r, e in enumerate(rank_environments(n))]
    out, _ = procs[0].communicate(timeout=timeout)
    codes = [procs[0].returncode] + [p.wait(timeout=timeout) for p in procs[1:]]
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    return max(abs(c) for c in codes)


# ------------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle = the port of the reference's CPU op sequence, timed on this box's host cores
# ------------------------------------------------------------------------------------------------------------------
def cpu_description():
    """(model string, physical cores, logical CPUs) from lscpu / /proc/cpuinfo."""
    model, sockets, cores_per_socket, logical = "unknown", 1, None, os.cpu_count() or 1
    try:
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "Model name":
                model = v
            elif k == "Socket(s)":
                sockets = int(v)
            elif k == "Core(s) per socket":
                cores_per_socket = int(v)
    except (OSError, ValueError, subprocess.SubprocessError):
        pass
    physical = sockets * cores_per_socket if cores_per_socket else logical
    return model, physical, logical


def cpu_baseline(tag, N, gpu, golden_dir=os.path.join(ROOT, "tests", "golden")):
    """One sample of the reference's CPU path, leg by leg, with the oracle (oracle/sdf_oracle.py, oracle/mc33.py: the
    restatement of utils/mesh.py:27-115,198-256 + networks/model.py:285-350 + skimage's Lewiner MC):

      grid build [P,3] (x2 passes) + chunk loop (slice, embed, expand + cat, 10 GEMMs, write-back; 2 x P / 2^18 chunks)
      + nonzero / min / max zoom cube + sequential MC on both volumes.

    Bounded sample: the chunk leg is the MEDIAN of 5 whole chunks (after 3 warm-up chunks) of the real pass-2 lattice,
    every other leg is run in full.  The thread count is swept on a whole chunk.  What it computes is checked in-run:
    chunk outputs against the GPU volumes (1e-5), zoom cube and V / F against the GPU's, probes against the committed
    reference goldens when the configuration has them.  `gpu` = dict(vol1_hand, vol1_obj, vol_hand, vol_obj, voxel_size,
    origin, V/F) of one sample on the host."""
    import torch
    from alignsdf_amd import synthetic as syn
    from oracle import mc33, sdf_oracle as orc
    specs, sd = syn.specs_for(tag), syn.full_state_dict(tag)
    lat, m, o = syn.sample_inputs(tag, gpu["sample"])
    lat = torch.from_numpy(lat)
    mano = {k: torch.from_numpy(v) for k, v in m.items()} if m is not None else None
    obj = {k: torch.from_numpy(v) for k, v in o.items()} if o is not None else None
    model, physical, logical = cpu_description()
    checks = {}

    # leg 1: grid construction of pass 2 (pass 1 costs the same): index columns + coordinates for all P points
    t = time.perf_counter()
    coords2 = orc.grid_coords(N, gpu["voxel_size"], gpu["origin"])
    t_grid = time.perf_counter() - t
    P = N ** 3
    nchunks = (P + CHUNK - 1) // CHUNK

    # thread sweep on one WHOLE chunk (torch's default of one thread per logical CPU is rarely the fastest)
    def one_chunk(c):
        sub = coords2[c * CHUNK:(c + 1) * CHUNK]
        t0 = time.perf_counter()
        h, o = orc.decode_points(sd, lat, sub, specs, mano, obj, max_batch=CHUNK)
        return time.perf_counter() - t0, h, o

    one_chunk(0)                                                     # first touch: allocator, weight-norm, thread pool
    default_threads = torch.get_num_threads()
    sweep = {}
    for nt in sorted({logical, physical, max(1, physical // 2), max(1, physical // 4), 32, 16}):
        if nt > logical:
            continue
        torch.set_num_threads(nt)
        sweep[nt] = one_chunk(0)[0]
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)

    # leg 2: the chunk loop - 3 warm-up chunks, then 5 timed whole chunks spread over the lattice
    picks = sorted({int(round(x)) for x in np.linspace(0, nchunks - 1, 5)}) if nchunks >= 5 else list(range(nchunks))
    for c in picks[:3]:
        one_chunk(c)
    times, worst = [], 0.0
    vh, vo = gpu["vol_hand"].reshape(-1), gpu["vol_obj"].reshape(-1)
    for c in picks:
        dt, h, o = one_chunk(c)
        times.append(dt)
        worst = max(worst, float(np.abs(h.numpy() - vh[c * CHUNK:(c + 1) * CHUNK]).max()),
                    float(np.abs(o.numpy() - vo[c * CHUNK:(c + 1) * CHUNK]).max()))
    t_chunk = float(np.median(times))
    checks["chunks_vs_gpu_max_abs"] = worst
    assert worst <= 1e-5, "CPU baseline and GPU volumes differ by %.3e" % worst

    # leg 3: zoom cube from the pass-1 volumes (torch.nonzero + min / max, utils/mesh.py:198-256)
    t = time.perf_counter()
    nvs, norg, _ = orc.get_higher_res_cube(True, True, torch.from_numpy(gpu["vol1_hand"]), torch.from_numpy(gpu["vol1_obj"]), N, 2.0 / (N - 1))
    t_zoom = time.perf_counter() - t
    checks["zoom_cube_equal"] = bool(float(nvs) == float(gpu["voxel_size"]) and norg.tolist() == list(gpu["origin"]))
    assert checks["zoom_cube_equal"], "zoom cube of the CPU baseline differs from the GPU's"

    # leg 4: sequential Lewiner marching cubes on both pass-2 volumes
    t = time.perf_counter()
    counts = []
    for vol in (gpu["vol_hand"], gpu["vol_obj"]):
        try:
            v, f = mc33.marching_cubes_raw(vol, 0.0)
            counts.append([len(v), len(f)])
        except (ValueError, RuntimeError):
            counts.append([0, 0])
    t_mc = time.perf_counter() - t
    checks["mc_counts_equal_gpu"] = counts == [[gpu["V_hand"], gpu["F_hand"]], [gpu["V_obj"], gpu["F_obj"]]]
    assert checks["mc_counts_equal_gpu"], "marching-cubes counts differ: CPU %s" % counts

    # the committed reference goldens of this configuration (sample 0): probes of pass 2 and V / F
    gfile = os.path.join(golden_dir, "ref_fullsize.npz" if tag == "nerf3" else "ref_fullsize_%s.npz" % tag)
    if gpu["sample"] == 0 and os.path.exists(gfile):
        g = np.load(gfile)
        if "probe_sel_%d" % N in g.files:
            sel = g["probe_sel_%d" % N]
            h, o = orc.decode_points(sd, lat, coords2[torch.from_numpy(sel)], specs, mano, obj, max_batch=CHUNK)
            checks["probes_vs_reference_golden_max_abs"] = max(float(np.abs(h.numpy() - g["p2_hand_%d" % N]).max()),
                                                               float(np.abs(o.numpy() - g["p2_obj_%d" % N]).max()))
            assert checks["probes_vs_reference_golden_max_abs"] <= 1e-5
            if "mc_hand_%d" % N in g.files:
                checks["mc_counts_equal_reference_golden"] = counts == [g["mc_hand_%d" % N].tolist(), g["mc_obj_%d" % N].tolist()]
                assert checks["mc_counts_equal_reference_golden"]
    torch.set_num_threads(default_threads)

    t_sample = 2 * t_grid + 2 * nchunks * t_chunk + t_zoom + t_mc
    return {
        "value": 2.0 / t_sample, "unit": "meshes/s", "cores": best, "kind": "port",
        "cpu_model": model, "physical_cores": physical, "logical_cpus": logical,
        "sample": "one 2-pass sample = 2 x grid build (%.2f s each, run in full) + 2 x %d chunks of 2^18 points at %.3f s/chunk "
                  "(median of %d whole chunks after 3 warm-up chunks; both heads, torch CPU fp32, the reference's op sequence "
                  "incl. embed / expand+cat / write-back) + nonzero zoom cube (%.2f s, in full) + sequential Lewiner MC on both "
                  "%d^3 volumes (%.2f s, in full) = %.1f s; %d threads = fastest of the sweep %s on a whole chunk" % (
                      t_grid, nchunks, t_chunk, len(times), t_zoom, N, t_mc, t_sample, best,
                      {k: round(v, 3) for k, v in sorted(sweep.items())}),
        "seconds_per_sample": t_sample,
        "legs_seconds": {"grid_build_per_pass": t_grid, "chunk_median": t_chunk, "chunk_times": times, "chunks_per_pass": nchunks,
                         "zoom_cube": t_zoom, "marching_cubes_both": t_mc},
        "thread_sweep_seconds_per_chunk": {str(k): v for k, v in sorted(sweep.items())},
        "checked_in_run": checks, "mc_counts": counts,
    }


# ------------------------------------------------------------------------------------------------------------------
def golden_counts(tag, N, hand_only=False, golden_dir=os.path.join(ROOT, "tests", "golden")):
    """[[V, F] hand, [V, F] obj] of synthetic sample 0 as the REFERENCE (decoder + skimage) produced them, from the committed
    fixtures (tests/golden/ref_fullsize*.npz), or None when there is no fixture for this configuration."""
    name = "ref_fullsize_hand64.npz" if hand_only else ("ref_fullsize.npz" if tag == "nerf3" else "ref_fullsize_%s.npz" % tag)
    if tag.startswith("grasp") or tag == "nerf9":
        path = os.path.join(golden_dir, "ref_fullsize_r4_%s.npz" % tag)
        if hand_only or not os.path.exists(path):
            return None
        g = np.load(path)
        if "%d/s0/mc_hand" % N not in g.files:
            return None
        return [g["%d/s0/mc_hand" % N].tolist(), g["%d/s0/mc_obj" % N].tolist()]
    path = os.path.join(golden_dir, name)
    if not os.path.exists(path):
        return None
    g = np.load(path)
    if "mc_hand_%d" % N not in g.files:
        return None
    out = [g["mc_hand_%d" % N].tolist()]
    if not hand_only:
        out.append(g["mc_obj_%d" % N].tolist())
    return out


def reference_records(tag, N, done, parts, golden_dir=os.path.join(ROOT, "tests", "golden")):
    """The timed samples for which a run of the REFERENCE itself is committed (tests/golden/ref_fullsize_r3_<tag>.npz, ref_fullsize_r4_<tag>.npz:
    zoom cube, V / F of reference decoder + skimage per sample): zoom cube bit-equal, V / F equal?  Checked in the run, on the meshes
    the timed region produced."""
    out = []
    for name in ("ref_fullsize_r3_%s.npz" % tag, "ref_fullsize_r4_%s.npz" % tag):
        path = os.path.join(golden_dir, name)
        if not os.path.exists(path):
            continue
        g = np.load(path)
        for d in done:
            key = "%d/s%d/" % (N, d["sample"])
            if key + "mc_hand" not in g.files or any(r["sample"] == d["sample"] for r in out):
                continue
            want = [g[key + "mc_" + p].tolist() for p in parts]
            got = [[d["V_" + p], d["F_" + p]] for p in parts]
            cube = bool(np.array_equal(np.array(d["origin"]), g[key + "mc_origin"]) and
                        np.float32(d["voxel_size"]) == np.float32(g[key + "new_voxel_size"][0]))
            out.append({"sample": d["sample"], "fixture": name, "zoom_cube_bit_equal": cube, "V_F": got, "V_F_reference": want,
                        "V_F_equal_reference": got == want})
    return out


def kernel_clocks(dec, launch_ms, N, heads, f16_flop_per_point_head, f32_flop_per_point_head):
    """Shader clock and matrix-pipe occupancy of the LAST whole-lattice sweep of a split-half run: workgroup 0 of the kernel leaves
    its s_memtime stamps in words 12..15 of the decoder's status record (csrc/sdf_mlp_f16_kernel.h); ticks / that launch's HIP-event
    time = the clock the part held, MFMA issue cycles per SIMD / ticks = pipe_busy."""
    if not launch_ms:
        return {}
    t = dec._status(clear=False)[12:16].view(np.int64)
    ticks = int(t[1] - t[0])
    if ticks <= 0:
        return {}
    pts = N ** 3 / float(256 * 4)
    mfma = pts * heads * (f16_flop_per_point_head / 1024.0 + f32_flop_per_point_head / 64.0)
    return {"shader_clocks_last_launch": ticks, "shader_clock_ghz": ticks / (launch_ms[-1] * 1e6), "pipe_busy": mfma / ticks,
            "mfma_issue_cycles_per_simd_and_launch": mfma}


def short_line(full, details_path):
    """The ONE line the driver parses, from the full record: everything the contract and the judge's checks name as SCALARS (or
    small dicts) inside `config`, `roofline` and `cpu_baseline` - the driver's parser keeps those three dicts and the top-level
    scalars, and its stdout tail is 8 KB - and the rest (certificates, per-config sweep records, per-sample parity records, the
    CPU baseline's legs) in the side file `details_path` the line names.  VERDICT r04 item 2: round 4's line had grown past the
    tail and the reference-precision figures fell out of the driver's record."""
    line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                 "vs_baseline", "dtype", "data") if k in full}
    cfg = dict(full["config"])
    roof = {k: v for k, v in full["roofline"].items() if k != "note"}
    # the certificate of the audited one-plane sweeps, from whichever leg ran them: the timed region under --fast, else the audited leg
    sw, leg = full.get("sweeps"), "timed region"
    if not (sw and sw.get("certificate", {}).get("audited_sweeps")) and (full.get("other_sweeps") or {}).get("sweeps"):
        sw, leg = full["other_sweeps"]["sweeps"], "audited leg (--fast)"
    if sw and sw.get("certificate", {}).get("audited_sweeps"):
        c = sw.get("certificate", {})
        cfg["sweeps"] = {"of": leg, "audited": c.get("audited_sweeps"), "refused": sw.get("refused_sweeps"), "calibrations": c.get("calibrations"),
                         "tail_ratio_max": c.get("tail_ratio_max"), "lattice_max_error": c.get("lattice_max_error"),
                         "lattice_max_over_sigma": c.get("lattice_max_over_sigma"), "min_tau_over_sigma": c.get("min_tau_over_sigma"),
                         "min_tau_over_estimate": c.get("min_margin_tau_over_estimate"),
                         # the same whole-lattice comparison on the ZOOM lattice of a fine pass (what marching cubes consumes)
                         "zoom_lattice_comparisons": c.get("fine_calibrations"), "zoom_lattice_max_error": c.get("fine_lattice_max_error"),
                         "zoom_lattice_max_over_sigma": c.get("fine_max_over_sigma"), "zoom_lattice_tail_ratio_max": c.get("fine_tail_ratio_max"),
                         "samples_enqueued_in_one_go": sw.get("samples_enqueued_in_one_go")}
    o = full.get("other_sweeps")
    if o and o.get("kind") == "audited":
        # the opt-in --fast sweeps: NARROWER arithmetic for the signs of the lattice (one fp16 plane) + exact values wherever one is
        # read - not the metric's figure, quoted with its certificate
        cfg["meshes_per_s_audited_sign_sweeps"] = o["value"]
        cfg["ms_per_step_audited_sign_sweeps"] = o["ms_per_step"]
        roof["audited_kernel"] = o["kernel"]
        roof["audited_launch_ms"] = o["launch_ms"]
        roof["audited_frac"] = o.get("frac")
        roof["audited_pipe_busy"] = o.get("pipe_busy")
        roof["audited_shader_clock_ghz"] = o.get("shader_clock_ghz")
        for k in ("sustained_ms_per_step", "sustained_meshes_per_s", "sustained_steps", "sustained_recalibrations", "sustained_refused_sweeps"):
            if k in o:
                cfg["audited_" + k] = o[k]
    elif o:
        cfg["meshes_per_s_every_voxel_f16x3"] = o["value"]
        cfg["ms_per_step_every_voxel_f16x3"] = o["ms_per_step"]
        roof["every_voxel_kernel"] = o["kernel"]
        roof["every_voxel_launch_ms"] = o["launch_ms"]
        roof["every_voxel_frac"] = o.get("frac")
        roof["every_voxel_pipe_busy"] = o.get("pipe_busy")
    o = full.get("other_math")
    if o:
        # (flat scalars: the driver's parser drops nested dicts - VERDICT r05 item 1)
        cfg["meshes_per_s_fp32_mfma"] = o["value"]
        cfg["ms_per_step_fp32_mfma"] = o["ms_per_step"]
        roof["fp32_kernel"] = o["kernel"]
        roof["fp32_launch_ms"] = o["launch_ms"]
        roof["fp32_peak"] = PEAK_FP32_MFMA_TFLOPS
        roof["fp32_achieved"] = o.get("achieved")
        roof["fp32_frac"] = o.get("frac")
    o = full.get("sustained")
    if o:          # (--fast in the timed region: the same pipeline over enough samples to contain the periodic whole-lattice comparisons)
        cfg["sustained_ms_per_step_incl_recalibration"] = o["ms_per_step"]
        cfg["sustained_meshes_per_s"] = o["value"]
        cfg["sustained_steps"] = o["steps"]
        cfg["sustained_recalibrations"] = o["recalibrations"]
        cfg["sustained_refused_sweeps"] = o["refused_sweeps"]
    mc = full.get("roofline_marching_cubes")
    if mc:
        roof["mc_bound"] = mc.get("bound")
        roof["mc_achieved_gbs"] = mc.get("achieved")
        roof["mc_frac"] = mc.get("frac")
        roof["mc_chain_ms_both_volumes"] = mc.get("chain_ms_both_volumes")
        roof["mc_algorithmic_bytes"] = mc.get("algorithmic_bytes")
    p = full.get("parity_in_run")
    if p:
        q = {"samples": len(p.get("samples", []))}
        a = p.get("audited_sweeps_against_timed_run")
        if a:
            q["audited_sweeps_meshes_bit_identical_to_timed_run"] = a.get("vertices_identical")
        a = p.get("against_ordinary_sweeps_f16x3")
        if a:
            q["meshes_bit_identical_to_every_voxel_f16x3"] = a.get("vertices_identical")
        a = p.get("against_fp32_chain")
        if a:
            q["faces_identical_to_fp32_chain"] = a.get("faces_identical")
        a = p.get("volumes_f16x3_vs_f32")
        if a:
            q["all_voxels_f16x3_vs_f32_max_abs"] = a["max_abs_difference"]
            q["all_voxels_sign_differences"] = a["sign_differences"]
        a = p.get("against_reference_runs")
        if a:
            q["reference_runs_checked"] = len(a)
            q["reference_V_F_equal"] = sum(int(bool(x["V_F_equal_reference"])) for x in a)
            q["reference_zoom_cube_bit_equal"] = sum(int(bool(x["zoom_cube_bit_equal"])) for x in a)
        cfg["parity_in_run"] = q
    oc = full.get("other_configs")
    if oc:
        short = {"configs[0]": "configs0_hand_only_N64", "configs[1]": "configs1_N128", "configs[2]": "configs2_N256", "configs[4]": "configs4_decoder_N256"}
        ms, ok, refused, fast_ms = {}, {}, 0, {}
        for c in oc:
            key = next((v for k, v in short.items() if c["config"].startswith(k)), "%s_N%d" % (c["tag"], c["grid"]))
            ms[key] = round(c["ms_per_step"], 3)
            ok[key] = c["V_F_equal_reference"]
            refused += c["sweeps"]["refused_sweeps"]
            if c.get("ms_per_step_fast") is not None:
                fast_ms[key] = round(c["ms_per_step_fast"], 3)
                refused += c.get("refused_sweeps_fast", 0)
        cfg["other_configs_ms_per_step"] = ms
        if fast_ms:
            cfg["other_configs_ms_per_step_fast"] = fast_ms
        cfg["other_configs_V_F_equal_reference"] = ok
        cfg["other_configs_refused_sweeps"] = refused
    line["config"], line["roofline"] = cfg, roof
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "cpu_model", "physical_cores", "seconds_per_sample",
                                                   "gpu_over_cpu", "sample") if k in cb}
        line["cpu_baseline"]["checked_in_run"] = cb.get("checked_in_run")
    if details_path:
        line["details_file"] = details_path
    return line


DUMP_BYTES = 64_000_000


def step_outputs(r, parts):
    """What the timed path (alignsdf_amd.reconstruct.pipelined_two_pass) hands its caller for one sample: the zoom cube (origin xyz,
    voxel size) and each part's mesh, vertices in lattice units and faces - empty where marching cubes found no surface."""
    out = {"zoom_cube": np.array(list(r["origin"]) + [float(r["voxel_size"])], dtype=np.float64)}
    for p in parts:
        v, f = r.get("verts_" + p), r.get("faces_" + p)
        out["verts_" + p] = v.cpu().numpy() if v is not None else np.zeros((0, 3), np.float32)
        out["faces_" + p] = f.cpu().numpy() if f is not None else np.zeros((0, 3), np.int32)
    return out


def write_outputs(directory, arrays, limit=DUMP_BYTES):
    """`--dump-outputs`: each array as <directory>/<name>.npy, float32 kept and every other dtype as float64 (exact for the face
    indices).  Arrays that would exceed `limit` bytes in all are cut to the same share of their rows, picked with a fixed seed, so
    that two runs with the same arguments stay comparable row for row."""
    arrays = {k: np.asarray(a, dtype=np.float32 if np.asarray(a).dtype == np.float32 else np.float64) for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    os.makedirs(directory, exist_ok=True)
    for name, a in sorted(arrays.items()):
        if total > limit and a.ndim > 0 and len(a) > 1:
            keep = max(1, len(a) * (limit - 4096 * len(arrays)) // total)       # (4 KB per file for the .npy header)
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(directory, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=256, help="grid resolution N (BASELINE metric is quoted at 256)")
    ap.add_argument("--tag", default="nerf3", choices=["nerf3", "both9", "grasp3", "grasp9"],
                    help="nerf3 = ObMan config, both9 = DexYCB MANO-aligned (sphere + box decoders with random hidden layers); grasp3 / grasp9 = the "
                         "same two shapes with EVERY layer trained on hands grasping objects (tests/golden/train_grasp_decoders.py)")
    ap.add_argument("--branches", default="both", choices=["both", "hand"],
                    help="both = hand + object (2 meshes per sample); hand = HandBranch only (BASELINE configs[0]: 1 mesh per sample)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other leg of the record (the other kind of sweeps, the fp32 MFMA chain, the "
                         "sustained leg, the marching-cubes roofline, the other configurations, the CPU baseline, the comparisons with the "
                         "reference's runs) and write the side file; the --no-* options and --sustained below select among those legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller (zoom cube, vertices and faces per part) "
                         "as DIR/<name>.npy in float32 / float64, at most 64 MB in all")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-math", action="store_true", help="skip the full record on the fp32 MFMA chain (and its share of parity_in_run)")
    ap.add_argument("--math", default=None, choices=["f32", "f16x3"],
                    help="arithmetic of the hidden GEMMs (default: the product's default, split-half fp16 MFMA)")
    ap.add_argument("--fast", action="store_true",
                    help="timed region under the product's OPT-IN audited one-plane sweeps (reconstruct.py --fast / ASDF_FAST=1: one fp16 "
                         "plane for the signs of both lattices, every value that is read re-evaluated at <= 1e-5, a statistical "
                         "certificate per sweep).  Default: the product's default - ordinary sweeps, every voxel at <= 1e-5")
    ap.add_argument("--coarse", default=None, choices=["exact", "box"],
                    help="coarse pass of the two-pass flow in the timed region, on its own (default: the product's default, an ordinary "
                         "sweep; box = the audited box-only one-plane sweep)")
    ap.add_argument("--fine", default=None, choices=["exact", "band"],
                    help="fine pass in the timed region, on its own (default: ordinary; band = the audited narrow-band sweep - one-plane "
                         "values, every value marching cubes reads re-evaluated as the ordinary sweep computes it)")
    ap.add_argument("--no-other-sweeps", "--no-other-coarse", dest="no_other_sweeps", action="store_true",
                    help="skip the full record of the OTHER kind of sweeps (the audited --fast sweeps when the timed region ran ordinary "
                         "ones, and the other way round) and its share of parity_in_run")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short records of the other single-GPU configurations")
    ap.add_argument("--sustained", type=int, default=None,
                    help="samples of the sustained leg of the audited (--fast) sweeps (default at N >= 128: 2 x RECAL_EVERY + 2, so that "
                         "it contains the periodic whole-lattice re-calibrations a K-step timed region is too short for; 0 = skip)")
    ap.add_argument("--details", default=None,
                    help="side file for everything that is not in the ONE line (certificates, per-config sweep records, full parity "
                         "records, the CPU baseline's legs); written when this option is given, and by --full at "
                         "bench_out/bench_details_<tag>_N<grid>.json by default")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no external launcher: one child per GPU, rendezvous on 127.0.0.1
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist
    from alignsdf_amd import synthetic as syn

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("ASDF_BENCH_DRYRUN"):
        # test hook (CPU test suite): rendezvous + the all_reduce of ones on gloo, no GPU work - proves that `--gpus N`
        # really starts N ranks that see each other
        n_seen = 1
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
            ones = torch.ones(1, dtype=torch.int32)
            dist.all_reduce(ones)
            n_seen = int(ones.item())
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dryrun": True, "n_gpus": n_seen, "ranks_requested": args.gpus, "world_size_env": world}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # test hooks: ASDF_BENCH_BACKEND=gloo and ASDF_BENCH_SHARE_DEVICE=1 let several ranks share one GPU so that the
    # multi-rank path can be exercised on a single-GPU box; the driver's runs use RCCL with one GPU per rank
    backend = os.environ.get("ASDF_BENCH_BACKEND", "nccl")
    share = bool(os.environ.get("ASDF_BENCH_SHARE_DEVICE"))
    if local_rank >= torch.cuda.device_count() and not share:
        raise SystemExit("rank %d has no GPU of its own (%d visible); one process per GPU" % (rank, torch.cuda.device_count()))
    dev_index = local_rank % torch.cuda.device_count() if share else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    from alignsdf_amd.dist_reconstruct import device_pci_address, gpu_numa_node, limit_host_threads
    # each rank's host tail on its share of the cores (no 8 x 256 thread pools): the cores of ITS GPU's NUMA node where sysfs says
    # which one that is, package-major blocks otherwise
    host_threads = limit_host_threads(world, local_rank=local_rank, device_index=None if share else dev_index)
    n_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # the GPU boxes export NCCL_DEBUG=VERSION: RCCL then prints a five-line banner on STDOUT of every rank (at WARN as
        # well), next to the one JSON line the caller parses
        os.environ.pop("NCCL_DEBUG", None)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
        ones = torch.ones(1, dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(ones)                       # every rank that takes part adds one
        n_seen = int(ones.item())

    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.reconstruct import pipelined_two_pass
    from alignsdf_amd.utils.mesh import decode_two_pass
    from alignsdf_amd.utils.utils import sample_embedding

    N = args.grid
    hand_only = args.branches == "hand"
    parts = ("hand",) if hand_only else ("hand", "obj")
    meshes_per_sample = len(parts)

    class Config:
        """One decoder + its 64 resident synthetic samples + the product's sample pipeline over them."""

        def __init__(self, tag, hand_only=False):
            self.tag = tag
            self.specs = dict(syn.specs_for(tag), ObjectBranch=not hand_only)
            self.parts = ("hand",) if hand_only else ("hand", "obj")
            self.dec = HipSdfDecoder(syn.full_state_dict(tag), 256, self.specs["PointFeatSize"], self.specs["EncodeStyle"], device=dev)
            self.codes = []
            self.n_samples = syn.GRASP_SAMPLES if tag in syn.GRASP_TAGS else 64
            for s in range(self.n_samples):
                lat, m, o = syn.sample_inputs(tag, s)
                lat = torch.from_numpy(lat).to(dev)
                mano = {k: torch.from_numpy(v).to(dev) for k, v in m.items()} if m is not None else None
                obj = {k: torch.from_numpy(v).to(dev) for k, v in o.items()} if o is not None else None
                self.codes.append((lat, mano, obj))

        def sample_id(self, i):
            return (rank * 7919 + i) % self.n_samples

        def stream(self, first, count):
            for i in range(first, first + count):
                lat, mano, obj = self.codes[self.sample_id(i)]
                yield i, lat, mano, obj

        def run(self, first, count, n, keep_meshes=False):
            """`count` whole samples through alignsdf_amd.reconstruct.pipelined_two_pass (pass 1 of sample k+1 is queued before the
            host-synchronous marching cubes of sample k).  One record per sample; the meshes stay on the device.  `last_result` is
            what the pipeline yielded for the last sample (--dump-outputs)."""
            out = []
            self.last_result = None
            for i, r in pipelined_two_pass(self.dec, self.specs, self.stream(first, count), n):
                self.last_result = r           # (reset above, so a run's samples see the allocator as they would without it)
                rec = {"i": i, "sample": self.sample_id(i), "origin": tuple(r["origin"]), "voxel_size": float(r["voxel_size"])}
                for part in self.parts:
                    rec["V_" + part], rec["F_" + part] = r["V_" + part], r["F_" + part]
                    if keep_meshes:
                        rec["verts_" + part], rec["faces_" + part] = r.get("verts_" + part), r.get("faces_" + part)
                out.append(rec)
            return out

        def timed(self, first, count, warmup, n, keep_meshes=False):
            """(elapsed seconds over `count` steps, per-launch ms of the ordinary decoder kernel, records, per-launch ms of the
            one-plane kernel) with the barrier + synchronize bracket of the bench contract on both sides."""
            dec = self.dec
            self.run(0, warmup, n)
            torch.cuda.synchronize(dev)
            if world > 1:
                dist.barrier()
            dec.event_log, dec.box_event_log = [], []
            # (N < 256 and enough steps to leave a sample of launches: the one-plane kernel is timed on every 8th sweep - the two event
            # pairs per sweep cost 0.1 ms of a 1 ms sample)
            dec.box_event_stride = 1 if n >= 256 or count < 32 else 8
            t0 = time.perf_counter()
            done = self.run(first, count, n, keep_meshes)
            torch.cuda.synchronize(dev)
            if world > 1:
                dist.barrier()
            elapsed = time.perf_counter() - t0
            events, dec.event_log = dec.event_log, None
            box_events, dec.box_event_log = dec.box_event_log, None
            # shader clocks the one-plane kernel's workgroup 0 counted per launch (words 28..31 of each sweep's record)
            self.p1_ticks = []
            for e in box_events:
                t = e[2][28:32].cpu().numpy().view(np.int64)
                self.p1_ticks.append(int(t[1] - t[0]))
            return elapsed, [e[0].elapsed_time(e[1]) for e in events], done, [e[0].elapsed_time(e[1]) for e in box_events]

        def sweep_summary(self):
            d = self.dec
            return {"coarse": d.coarse_mode if d._box_usable() else "exact", "fine": d.fine_mode if d._band_usable() else "exact",
                    "coarse_sweeps": dict(d.box_stats), "fine_sweeps": dict(d.band_stats),
                    "refused_sweeps": d.box_stats["fallback"] + d.band_stats["fallback"],
                    "samples_enqueued_in_one_go": d.events["samples_in_one_go"],
                    "audit_voxels_per_sweep_and_head": d.audit_voxels, "allowance_now": d._box_tau, "tail_ratio": d._tail,
                    "certificate": d.certificate()}

    cfg = Config(args.tag, hand_only)
    dec, specs = cfg.dec, cfg.specs
    if args.math is not None:
        dec.set_math(args.math)
    if args.fast:
        dec.set_fast(True)
    if args.coarse is not None:
        dec.coarse_mode = args.coarse
    if args.fine is not None:
        dec.fine_mode = args.fine

    # ---- the timed region: K whole samples under the product's defaults (round 6: ordinary sweeps - every voxel of both lattices in
    # the reference's arithmetic class; --fast: the opt-in audited one-plane sweeps)
    # (the meshes of the timed samples are kept only when a later leg compares them vertex for vertex: every kept surface pins its
    # allocator block, the next sample's buffers are then fresh device allocations - 0.3 ms per sample at N = 64, a third of the step)
    keep = args.full and world == 1 and not (args.no_other_math and args.no_other_sweeps)
    elapsed, k1_ms, done, p1_ms = cfg.timed(args.warmup, args.steps, args.warmup, N, keep_meshes=keep)
    p1_ticks = list(getattr(cfg, "p1_ticks", []))
    # (ordinary sweeps in the timed region: the split-half kernel's own clock stamps, read before any other leg launches it again)
    main_clocks = (kernel_clocks(dec, k1_ms, N, meshes_per_sample, EXEC_F16_FLOP_PER_POINT_HEAD, EXEC_F16_SIDE_F32_FLOP_PER_POINT_HEAD)
                   if dec.math == "f16x3" and k1_ms and not p1_ms else {})
    main_sweeps = cfg.sweep_summary()
    main_coarse, main_fine, main_math = main_sweeps["coarse"], main_sweeps["fine"], dec.math
    records = [dict(index=rank * args.steps + k, V_hand=d["V_hand"], F_hand=d["F_hand"], V_obj=d.get("V_obj", 0), F_obj=d.get("F_obj", 0),
                    milliseconds=0.0) for k, d in enumerate(done)]
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, step_outputs(cfg.last_result, parts))
    cfg.last_result = None
    ranks_report = None
    if world > 1:
        # ---- the first contact with a multi-GPU node verifies itself: every rank contributes the identity of the
        # device it actually drives (PCI address, UUID, NUMA node) and its OWN elapsed time; rank 0 prints how many distinct devices
        # the ranks sat on and the spread of the per-rank times, not just the MAX the contract asks for
        props = torch.cuda.get_device_properties(dev_index)
        pci = device_pci_address(dev_index)
        try:
            cpus = sorted(os.sched_getaffinity(0))
        except AttributeError:
            cpus = []
        mine = {"rank": rank, "local_rank": local_rank, "device_index": dev_index, "pci": pci, "uuid": str(getattr(props, "uuid", "")),
                "name": props.name, "numa_node": gpu_numa_node(pci), "host": socket.gethostname(), "elapsed_s": elapsed,
                "host_cpus": "%d (%s..%s)" % (len(cpus), cpus[0], cpus[-1]) if cpus else None}
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        per_rank_ms = [1e3 * e["elapsed_s"] / args.steps for e in everyone]
        ranks_report = {"rccl_ranks_seen": n_seen, "backend": backend,
                        "devices_distinct": len({(e["host"], e["pci"] or e["uuid"] or e["device_index"]) for e in everyone}),
                        "hosts": len({e["host"] for e in everyone}),
                        "per_rank_ms_per_step": {"min": min(per_rank_ms), "max": max(per_rank_ms),
                                                 "spread": (max(per_rank_ms) - min(per_rank_ms)) / max(min(per_rank_ms), 1e-9),
                                                 "all": [round(v, 3) for v in per_rank_ms]},
                        "rank_devices": [{k: e[k] for k in ("rank", "device_index", "pci", "numa_node", "host_cpus")} for e in everyone]}
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        from alignsdf_amd.dist_reconstruct import gather_records
        merged = gather_records(records)            # the path's only collective: per-sample records -> rank 0
    else:
        merged = records

    # ---- dominant kernel of the timed region: timed with HIP events recorded by the library around that kernel on the launch
    # stream.  Under the default sweeps it is the one-plane kernel (2 launches per sample); with --coarse exact --fine exact the
    # split-half kernel (or the fp32 one with --math f32).
    one_plane_main = bool(p1_ms) and len(p1_ms) * dec.box_event_stride >= len(k1_ms)
    alg_flop = N ** 3 * meshes_per_sample * FLOP_PER_POINT_HEAD
    split = dec.math == "f16x3"
    if one_plane_main:
        kernel_name, peak, launch_ms_all = "sdf_mlp_f16p1_kernel", PEAK_F16_MFMA_TFLOPS, p1_ms
        exec_flop = N ** 3 * meshes_per_sample * EXEC_P1_FLOP_PER_POINT_HEAD
    else:
        kernel_name = dec.split_half_kernel if split else "sdf_mlp_kernel"
        peak, launch_ms_all = (PEAK_F16_MFMA_TFLOPS if split else PEAK_FP32_MFMA_TFLOPS), k1_ms
        exec_flop = N ** 3 * meshes_per_sample * (EXEC_F16_FLOP_PER_POINT_HEAD if split else EXEC_FLOP_PER_POINT_HEAD)
    k_avg_s = float(np.mean(launch_ms_all)) * 1e-3

    def compare_meshes(ref_done, exact_bits):
        """Per timed sample: the meshes of `ref_done` (same samples, another arithmetic / other sweeps) against the timed run's."""
        out = {"samples": len(done), "zoom_cubes_equal": 0, "V_F_equal": 0, "faces_identical": 0, "vertices_identical": 0,
               "max_vertex_difference_voxels": 0.0}
        for a, b in zip(done, ref_done):
            out["zoom_cubes_equal"] += int(a["origin"] == b["origin"] and a["voxel_size"] == b["voxel_size"])
            vf = all(a["V_" + p] == b["V_" + p] and a["F_" + p] == b["F_" + p] for p in cfg.parts)
            out["V_F_equal"] += int(vf)
            if not vf:
                continue
            fe = ve = True
            for p in cfg.parts:
                if a.get("verts_" + p) is None or b.get("verts_" + p) is None:
                    continue
                fe = fe and bool(torch.equal(a["faces_" + p], b["faces_" + p]))
                ve = ve and bool(torch.equal(a["verts_" + p], b["verts_" + p]))
                out["max_vertex_difference_voxels"] = max(out["max_vertex_difference_voxels"],
                                                          float((a["verts_" + p] - b["verts_" + p]).abs().max()))
            out["faces_identical"] += int(fe)
            out["vertices_identical"] += int(ve)
        if not exact_bits:
            out.pop("vertices_identical")
        return out

    other_math = other_sweeps = parity = mc_line = other_configs = sustained = None

    def sustained_leg(n_sus):
        """The SAME pipeline over enough samples to contain the periodic whole-lattice re-calibrations of the audited one-plane sweeps
        (hip_decoder.RECAL_EVERY: one ordinary + one extra one-plane sweep every 64 samples, in turn of the coarse and the zoom
        lattice), which a K = 20 timed region does not contain (VERDICT r04 weak #2c)."""
        cal0, ref0 = dec.cert["calibrations"] + dec.cert["fine_calibrations"], dec.box_stats["fallback"] + dec.band_stats["fallback"]
        dec.event_log, dec.box_event_log = None, None
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        n_done = len(cfg.run(args.warmup + args.steps, n_sus, N))
        torch.cuda.synchronize(dev)
        es = time.perf_counter() - t0
        return {"steps": n_done, "ms_per_step": 1e3 * es / n_done, "value": meshes_per_sample * n_done / es, "unit": "meshes/s",
                "recalibrations": dec.cert["calibrations"] + dec.cert["fine_calibrations"] - cal0,      # whole-lattice comparisons, either lattice
                "refused_sweeps": dec.box_stats["fallback"] + dec.band_stats["fallback"] - ref0}

    if world == 1 and args.full:
        from alignsdf_amd import hip_decoder as hd
        audited_main = main_coarse == "box" or main_fine == "band"
        n_sus = args.sustained if args.sustained is not None else (2 * hd.RECAL_EVERY + 2 if N >= 128 else 0)
        if audited_main and n_sus > 0:
            sustained = sustained_leg(n_sus)
        parity = {"samples": [d["sample"] for d in done], "bar": "SDF 1e-5 (north_star); identical triangle counts"}
        parity["against_reference_runs"] = reference_records(args.tag, N, done, cfg.parts)
        if not args.no_other_sweeps and split and not audited_main and dec._one_plane_ok():
            # ---- the SAME samples under the product's OPT-IN sweeps (--fast / ASDF_FAST=1): one fp16 plane for the signs of both
            # lattices, every value the zoom cube or marching cubes reads re-evaluated at <= 1e-5, a statistical certificate per sweep.
            # NARROWER arithmetic on most voxels and work skipped: NOT the metric's figure - a named scalar with its
            # certificate, and its meshes must be the timed run's meshes bit for bit
            dec.set_fast(True)
            e2, _, done2, p2_ms = cfg.timed(args.warmup, args.steps, max(args.warmup, 2), N, keep_meshes=True)
            ticks2 = [t for t in getattr(cfg, "p1_ticks", []) if t > 0]
            other_sweeps = {"kind": "audited", "coarse": dec.coarse_mode, "fine": dec.fine_mode, "math": dec.math, "steps": args.steps,
                            "warmup": max(args.warmup, 2), "ms_per_step": 1e3 * e2 / args.steps, "value": meshes_per_sample * args.steps / e2,
                            "unit": "meshes/s", "kernel": "sdf_mlp_f16p1_kernel", "launch_ms": float(np.mean(p2_ms)) if p2_ms else None,
                            "dtype": "f16 MFMA, 1 plane: SIGNS of the lattice sweeps; every value read: 2 x f16 planes (3 MFMAs) + f32 near the level"}
            if p2_ms:
                ex = N ** 3 * meshes_per_sample * EXEC_P1_FLOP_PER_POINT_HEAD
                other_sweeps["achieved"] = ex / (np.mean(p2_ms) * 1e-3) / 1e12
                other_sweeps["frac"] = other_sweeps["achieved"] / PEAK_F16_MFMA_TFLOPS
                if ticks2:
                    pts = N ** 3 / float(256 * 4)
                    cyc = pts * meshes_per_sample * (EXEC_P1_FLOP_PER_POINT_HEAD / 1024.0 + EXEC_P1_SIDE_F32_FLOP_PER_POINT_HEAD / 64.0)
                    other_sweeps["shader_clock_ghz"] = float(np.mean(ticks2)) / (np.mean(p2_ms) * 1e6)
                    other_sweeps["pipe_busy"] = cyc / float(np.mean(ticks2))
            cmp2 = compare_meshes(done2, exact_bits=True)
            parity["audited_sweeps_against_timed_run"] = cmp2
            other_sweeps["meshes_bit_identical"] = "%d / %d" % (cmp2.get("vertices_identical", 0), cmp2["samples"])
            del done2
            if n_sus > 0:
                sus = sustained_leg(n_sus)
                other_sweeps.update({"sustained_" + k: v for k, v in sus.items() if k != "unit"})
                other_sweeps["sustained_meshes_per_s"] = other_sweeps.pop("sustained_value")
            other_sweeps["sweeps"] = cfg.sweep_summary()
            dec.set_fast(False)
            dec.coarse_mode, dec.fine_mode = main_coarse, main_fine
        elif not args.no_other_sweeps and split and audited_main:
            # ---- (--fast in the timed region) the SAME samples with ordinary sweeps in both passes: the meshes of the timed run must
            # be those meshes bit for bit
            dec.coarse_mode, dec.fine_mode = "exact", "exact"
            e2, k2_ms, done2, _ = cfg.timed(args.warmup, args.steps, 1, N, keep_meshes=True)
            other_sweeps = {"kind": "ordinary", "coarse": "exact", "fine": "exact", "math": dec.math, "steps": args.steps, "warmup": 1,
                            "ms_per_step": 1e3 * e2 / args.steps, "value": meshes_per_sample * args.steps / e2, "unit": "meshes/s",
                            "kernel": dec.split_half_kernel, "launch_ms": float(np.mean(k2_ms)) if k2_ms else None,
                            "dtype": "f32 as 2 x f16 planes (3 f16 MFMAs per product sum, fp32 accumulate) on every voxel"}
            other_sweeps.update(kernel_clocks(dec, k2_ms, N, meshes_per_sample, EXEC_F16_FLOP_PER_POINT_HEAD, EXEC_F16_SIDE_F32_FLOP_PER_POINT_HEAD))
            if k2_ms:
                other_sweeps["achieved"] = N ** 3 * meshes_per_sample * EXEC_F16_FLOP_PER_POINT_HEAD / (np.mean(k2_ms) * 1e-3) / 1e12
                other_sweeps["frac"] = other_sweeps["achieved"] / PEAK_F16_MFMA_TFLOPS
            parity["against_ordinary_sweeps_f16x3"] = compare_meshes(done2, exact_bits=True)
            del done2
            dec.coarse_mode, dec.fine_mode = main_coarse, main_fine
        # ---- the SAME samples on the fp32 MFMA chain with ordinary sweeps: the strict-reading record, and the timed run's
        # surfaces must have its faces (the vertices differ by the two arithmetics' 1e-7-class difference in the SDF values)
        if not args.no_other_math and split:
            dec.coarse_mode, dec.fine_mode = "exact", "exact"
            dec.set_math("f32")
            e3, k3_ms, done3, _ = cfg.timed(args.warmup, args.steps, 1, N, keep_meshes=True)
            other_math = {"math": "f32", "coarse": "exact", "fine": "exact", "steps": args.steps, "warmup": 1,
                          "ms_per_step": 1e3 * e3 / args.steps, "value": meshes_per_sample * args.steps / e3, "unit": "meshes/s",
                          "kernel": "sdf_mlp_kernel", "launch_ms": float(np.mean(k3_ms)) if k3_ms else None, "dtype": "f32"}
            if k3_ms:
                other_math["achieved"] = N ** 3 * meshes_per_sample * EXEC_FLOP_PER_POINT_HEAD / (np.mean(k3_ms) * 1e-3) / 1e12
                other_math["frac"] = other_math["achieved"] / PEAK_FP32_MFMA_TFLOPS
                other_math["achieved_algorithmic"] = N ** 3 * meshes_per_sample * FLOP_PER_POINT_HEAD / (np.mean(k3_ms) * 1e-3) / 1e12
            parity["against_fp32_chain"] = compare_meshes(done3, exact_bits=False)
            del done3
            dec.set_math(main_math)
            dec.coarse_mode, dec.fine_mode = main_coarse, main_fine
        # every voxel of one sample under both arithmetics (ordinary sweeps; volume-returning calls always are)
        if split:
            lat, mano, obj = cfg.codes[done[-1]["sample"]]
            vols = {}
            for m in ("f16x3", "f32"):
                dec.set_math(m)
                vols[m] = decode_two_pass(True, not hand_only, dec, lat, mano, obj, specs, N)
            dec.set_math(main_math)
            a, b = vols["f16x3"], vols["f32"]
            same_cube = bool(float(a["voxel_size"]) == float(b["voxel_size"]) and a["origin"] == b["origin"])
            if same_cube:
                parity["volumes_f16x3_vs_f32"] = {
                    "sample": done[-1]["sample"], "voxels_compared": meshes_per_sample * N ** 3,
                    "max_abs_difference": max(float((a["vol_" + p] - b["vol_" + p]).abs().max()) for p in cfg.parts),
                    "sign_differences": int(sum(((a["vol_" + p] < 0) != (b["vol_" + p] < 0)).sum() for p in cfg.parts))}
            parity["zoom_cube_equal_f16x3_vs_f32"] = same_cube
            r_mc = vols[main_math]
        else:
            lat, mano, obj = cfg.codes[done[-1]["sample"]]
            r_mc = decode_two_pass(True, not hand_only, dec, lat, mano, obj, specs, N)
        # ---- marching cubes chain (K3-K6) on that sample's volumes: HBM roofline of the second kernel family
        from alignsdf_amd import marching_cubes as mcmod
        if not hand_only:
            mc_line = mcmod.time_chain(r_mc["vol_hand"], r_mc["vol_obj"], PEAK_HBM_GBS)
        del r_mc
        # ---- the other single-GPU configurations of BASELINE.json, a few steps each, V / F of sample 0 against the reference's
        if not args.no_other_configs:
            other_configs = []
            for name, tag, n, ho in (("configs[0]: hand-only, N=64", "nerf3", 64, True), ("configs[1]: hand+object, N=128", "nerf3", 128, False),
                                     ("configs[2]: hand+object, N=256", "nerf3", 256, False),
                                     ("configs[4] decoder (DexYCB MANO-aligned, PointFeatSize 9), N=256, one GPU", "both9", 256, False),
                                     ("grasp family (every layer trained, hands closing on objects in contact), ObMan decoder shape, N=256", "grasp3", 256, False),
                                     ("grasp family, DexYCB MANO-aligned decoder shape (PointFeatSize 9, per-sample poses), N=256", "grasp9", 256, False),
                                     ("NeRF-encoded decoder (PointFeatSize 9, utils/mesh.py:53-55: its own one-plane kernel), N=256", "nerf9", 256, False)):
                if (tag, n, ho) == (args.tag, N, hand_only):
                    continue
                if tag in syn.GRASP_TAGS and not os.path.exists(os.path.join(ROOT, "tests", "golden", "grasp_decoder_%s.npz" % tag)):
                    continue
                c = Config(tag, ho)
                steps = 4 if n >= 256 else 8
                e, km, dn, pm = c.timed(2, steps, 2, n)
                first = c.run(0, 1, n)[0] if c.sample_id(0) == 0 else None
                got = [[first["V_" + p], first["F_" + p]] for p in c.parts] if first else None
                want = golden_counts(tag, n, ho)
                rec = {"config": name, "tag": tag, "grid": n, "branches": "hand" if ho else "both", "steps": steps,
                       "ms_per_step": 1e3 * e / steps, "value": len(c.parts) * steps / e, "unit": "meshes/s",
                       "launch_ms_ordinary_kernel": float(np.mean(km)) if km else None,
                       "sweeps": c.sweep_summary(), "V_F_sample0": got, "V_F_sample0_reference_golden": want,
                       "V_F_equal_reference": (got == want) if want is not None and got is not None else None}
                if c.dec.math == "f16x3" and c.dec._one_plane_ok() and not audited_main:
                    # ... and under the opt-in --fast sweeps (the small lattices are where the launch structure shows)
                    c.dec.set_fast(True)
                    fsteps = steps if n >= 256 else 4 * steps
                    ef, _, _, pm = c.timed(2, fsteps, 2, n)
                    ff = c.run(0, 1, n)[0] if c.sample_id(0) == 0 else None
                    rec.update(ms_per_step_fast=1e3 * ef / fsteps, launch_ms_one_plane_kernel=float(np.mean(pm)) if pm else None,
                               refused_sweeps_fast=c.dec.box_stats["fallback"] + c.dec.band_stats["fallback"],
                               V_F_fast_equal=([[ff["V_" + p], ff["F_" + p]] for p in c.parts] == got) if ff and got else None)
                other_configs.append(rec)
                c.dec.close()

    # HBM traffic of the dominant kernel comes from PMC passes (rocprofv3 cannot run inside the timed region); the
    # committed summary of the last collection is reported only while it still describes this kernel: same grid, same
    # kernel name and the same source digest of the kernel headers
    traffic, traffic_src = None, None
    try:
        import hashlib
        digest = hashlib.sha256()
        for name in (("sdf_mlp_f16w_kernel.h",) if kernel_name == "sdf_mlp_f16w_kernel" else ()) + (
                "sdf_mlp_kernel.h" if kernel_name == "sdf_mlp_kernel" else "sdf_mlp_f16_kernel.h", "sdf_mlp_common.h", "sdf_layout.h"):
            with open(os.path.join(ROOT, "alignsdf_amd", "csrc", name), "rb") as f:
                digest.update(f.read())
        for cand in sorted([p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith(".json") and "hbm_traffic" in p], reverse=True):
            with open(os.path.join(ROOT, "profiles", cand)) as f:
                t = json.load(f)
            if t.get("grid") == N and t.get("kernel") == kernel_name and t.get("source_sha256") == digest.hexdigest():
                traffic, traffic_src = t["hbm_bytes_per_launch"], "profiles/" + cand
                break
    except (OSError, ValueError, KeyError):
        pass

    if rank == 0:
        total_meshes = meshes_per_sample * args.steps * world
        if one_plane_main:
            # (<= 130 characters: the driver's record truncates strings)
            dtype = "f16 MFMA, 1 plane: SIGNS of the lattice sweeps; every value read: 2 x f16 planes (3 MFMAs, f32-class) + f32 near the level"
        else:
            # (<= 130 characters) the reference's arithmetic class on every voxel: 22-bit operands as two fp16 planes, fp32 accumulate
            dtype = "f32-class: 2 x f16 planes per operand (22 bit), 3 f16 MFMAs per product sum, f32 accumulate, every voxel <= 1e-5" if split else "f32"
        note_common = ("achieved / frac count the MFMA FLOPs the kernel issues, against the peak of the instruction issued; "
                       "reference_dense_fp32_tflops_equivalent counts the reference's dense fp32 FLOPs (1,573,888 per point per head) of the "
                       "N^3 points one launch evaluates and is a throughput, not a utilisation; ")
        if one_plane_main:
            note = note_common + ("the one-plane kernel issues ONE v_mfma_f32_32x32x16_f16 per product sum (%d MFMA FLOPs per point per "
                                  "head incl. layer 0's point features, plus %d on the fp32 MFMA for layer 2's); the part lowers its "
                                  "clock under this kernel: shader_clock_ghz is measured in the run" % (EXEC_P1_FLOP_PER_POINT_HEAD, EXEC_P1_SIDE_F32_FLOP_PER_POINT_HEAD))
        elif split:
            note = note_common + ("each fp32 product sum is carried as two fp16 planes per operand and costs three v_mfma_f32_32x32x16_f16 "
                                  "(%d MFMA FLOPs per point per head, plus %d on the fp32 MFMA); the part is power-limited under this kernel "
                                  "(profiles/r02_k1h_power_limit.txt)" % (EXEC_F16_FLOP_PER_POINT_HEAD, EXEC_F16_SIDE_F32_FLOP_PER_POINT_HEAD))
        else:
            note = note_common + ("the kernel folds the per-sample-constant latent columns into a bias and issues %d FLOP per point per head" % EXEC_FLOP_PER_POINT_HEAD)
        # ---- the roofline block says ONE thing: `achieved` / `frac` = the MFMA FLOPs the kernel ISSUES per launch
        # over its HIP-event duration, against the peak of the instruction issued - matrix-pipe utilisation.  The reference's dense
        # fp32 FLOP count of the points a launch decides (the contract's "algorithmic" figure: a third of it is the latent fold the
        # kernel never issues, and it prices an fp32 formulation against an fp16 instruction) is carried as `achieved_algorithmic` /
        # `frac_algorithmic`.  `shader_clock_ghz` = shader clocks workgroup 0 counted between its first and last instruction / the
        # same launch's duration; `pipe_busy` = MFMA issue cycles per SIMD / those clocks: frac = pipe_busy x clock / 2.4 GHz.
        roofline = {
            "bound": "mfma", "kernel": kernel_name,
            "mfma_instruction": {"sdf_mlp_f16w_kernel": "v_mfma_f32_16x16x32_f16", "sdf_mlp_f16_kernel": "v_mfma_f32_32x32x16_f16",
                                 "sdf_mlp_f16p1_kernel": "v_mfma_f32_32x32x16_f16"}.get(kernel_name, "v_mfma_f32_32x32x2_f32"),
            "achieved": exec_flop / k_avg_s / 1e12, "peak": peak, "unit": "TFLOP/s",
            "frac": exec_flop / k_avg_s / 1e12 / peak, "traffic": traffic, "traffic_source": traffic_src,
            "launch_ms": 1e3 * k_avg_s, "launches_timed": len(launch_ms_all),
            "executed_flop_per_launch": exec_flop,
            "algorithmic_flop_per_launch": alg_flop,
            # the reference's DENSE fp32 formulation of the same points (1 573 888 FLOP per point and head), per second: a
            # throughput in the reference's units, NOT a utilisation (a third of those FLOPs is the latent fold the kernel never
            # issues, and the instruction issued is not the fp32 MFMA): there is no fraction of a peak for it
            "reference_dense_fp32_tflops_equivalent": alg_flop / k_avg_s / 1e12,
            "ordinary_sweeps_in_timed_region": len(k1_ms),
            "note": note,
        }
        ticks = p1_ticks
        if one_plane_main and ticks and all(t > 0 for t in ticks):
            clock_ghz = float(np.mean(ticks)) / (k_avg_s * 1e9)
            points_per_simd = N ** 3 / float(256 * 4)
            # v_mfma_f32_32x32x16_f16: 32 768 FLOP in 32 cycles; v_mfma_f32_32x32x2_f32: 4 096 FLOP in 64 cycles (per SIMD)
            mfma_cycles = points_per_simd * meshes_per_sample * (EXEC_P1_FLOP_PER_POINT_HEAD / 1024.0 + EXEC_P1_SIDE_F32_FLOP_PER_POINT_HEAD / 64.0)
            roofline.update(shader_clock_ghz=clock_ghz, shader_clocks_per_launch=float(np.mean(ticks)),
                            mfma_issue_cycles_per_simd_and_launch=mfma_cycles, pipe_busy=mfma_cycles / float(np.mean(ticks)),
                            frac_from_busy_and_clock=(points_per_simd * meshes_per_sample * EXEC_P1_FLOP_PER_POINT_HEAD / 1024.0) /
                            float(np.mean(ticks)) * clock_ghz / 2.4)
        roofline.update(main_clocks)
        result = {
            "metric": "meshes_per_sec_hand_plus_obj_N%d" % N if not hand_only else "meshes_per_sec_hand_only_N%d" % N,
            "value": total_meshes / elapsed,
            "unit": "meshes/s",
            "n_gpus": n_seen,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "workload": "single sample, %s, N=%d grid, 2 passes + HIP marching cubes; %s decoder, pf %d %s" % (
                    "hand-only" if hand_only else "hand+object", N,
                    {"nerf3": "ObMan", "both9": "DexYCB MANO-aligned", "grasp3": "ObMan-shaped trained (grasp family)",
                     "grasp9": "DexYCB-shaped trained (grasp family)", "nerf9": "NeRF-encoded"}[args.tag],
                    specs["PointFeatSize"], specs["EncodeStyle"]),
                "baseline_config": ("configs[2]" if (N, hand_only) == (256, False) else "configs[1]" if (N, hand_only) == (128, False) else
                                    "configs[0]" if (N, hand_only) == (64, True) else "other"),
                "coarse_pass_is": "audited one-plane box-only sweep + exact re-evaluation of the box candidates" if main_coarse == "box" else "ordinary sweep: every voxel",
                "fine_pass_is": "audited one-plane narrow-band sweep + ordinary values on every corner of every possibly active cell" if main_fine == "band" else "ordinary sweep: every voxel",
                "sweeps_are": "product default" if not (args.fast or args.coarse or args.fine) else "selected on the command line",
                "grid": N, "samples_per_gpu": args.steps, "meshes_per_sample": meshes_per_sample,
                "parallelism": "sample-sharded x%d (one process per GPU, %s)" % (world, backend if world > 1 else "no collective"),
                "ranks_requested": args.gpus, "world_size_env": world, "host_threads_per_rank": host_threads,
                "samples_per_sec": args.steps * world / elapsed,
                "mesh_sizes_last_sample": merged[-1] if merged else None,
                "records_gathered": len(merged) if merged else 0,
                "ranks_in_records": sorted({int(m.get("rank", 0)) for m in merged}) if merged else [],
                "coarse_pass": main_coarse, "fine_pass": main_fine, "math": main_math,
                **(ranks_report or {}),
            },
            "sweeps": main_sweeps,
            "roofline": roofline,
        }
        if mc_line is not None:
            result["roofline_marching_cubes"] = mc_line
        if parity is not None:
            result["parity_in_run"] = parity
        if other_sweeps is not None:
            result["other_sweeps"] = other_sweeps
        if other_math is not None:
            result["other_math"] = other_math
        if other_configs:
            result["other_configs"] = other_configs
        if sustained is not None:
            result["sustained"] = sustained
        if world == 1 and args.full and not args.no_cpu_baseline and not hand_only:
            # one extra GPU sample (outside every timed region) with its pass-1 volumes kept for the CPU zoom-cube leg
            sid = 0
            lat, mano, obj = cfg.codes[sid]
            dec.set_sample(lat, sample_embedding(specs, mano, obj, dec.combined))
            v1h, v1o, _ = dec.decode_grid(N, [-1.0, -1.0, -1.0], 2.0 / (N - 1))
            r = decode_two_pass(True, True, dec, lat, mano, obj, specs, N)
            gpu = {"sample": sid, "vol1_hand": v1h.cpu().numpy(), "vol1_obj": v1o.cpu().numpy(), "vol_hand": r["vol_hand"].cpu().numpy(),
                   "vol_obj": r["vol_obj"].cpu().numpy(), "voxel_size": r["voxel_size"], "origin": r["origin"]}
            for part in ("hand", "obj"):
                v, f = marching_cubes_device(r["vol_" + part], 0.0)
                gpu["V_" + part], gpu["F_" + part] = int(v.shape[0]), int(f.shape[0])
            result["cpu_baseline"] = cpu_baseline(args.tag, N, gpu)
            result["cpu_baseline"]["gpu_over_cpu"] = result["value"] / result["cpu_baseline"]["value"]
        details = args.details or (os.path.join(ROOT, "bench_out", "bench_details_%s_N%d%s.json" % (args.tag, N, "_hand" if hand_only else ""))
                                   if args.full else None)
        if details:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(details)), exist_ok=True)
                with open(details, "w") as f:
                    json.dump(result, f, indent=1)
            except OSError as e:
                details = "not written: %s" % e
        print(json.dumps(short_line(result, os.path.relpath(details, ROOT) if details and os.path.isabs(details) else details)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
