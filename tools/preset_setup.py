"""What the per-feature scripts (second_round.py, rescue_round.py, extended_fill.py, anchor_modes.py) share: one bench preset as a GapFill
with its gaps set and the preset's libraries synthesised on the device; and what the scripts of the three after-pick rounds
(read_support.py, polish_fills.py, pair_span.py) share on top: their options, the off / on timing, the round's own time, the output."""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 150


def preset_setup(config, reads=0, gap_len=0, mp_reads=0, edit_flanks=None):
    """reads / gap_len: read records of the short-insert library / gap length (0: the preset's); mp_reads: read records of the preset's
    mate-pair library (IS 5000 / sd 500; 0: none); edit_flanks(flanks) -> flanks: the draft's flanks as the picker is to see them.
    Returns a namespace: gf, cfg (the short-insert library's), gaps, kk, gap_len, reads, libs [(name, IS mean, IS sd, read records,
    d_reads, d_recs, pull_mates)], truth(g) = the two strings a closed gap's sequence may equal (gf_synth_truth), pipeline(**flags)."""
    import bench
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    seed, slen, nscf, gps, glen, dreads, kk = bench.PRESETS[config]
    glen = gap_len or glen
    rep_p, rep_c = bench.REPEATS.get(config, (0, 50))

    def synth_cfg(is_mean, is_sd, lib_no):
        return GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                                 insert_mean=is_mean, insert_sd=is_sd, library=lib_no, repeat_period=rep_p, repeat_copies=rep_c)
    cfg = synth_cfg(300, 30, 0)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf = GapFill(0)
    gf.set_gaps(gaps, nscf, edit_flanks(flanks) if edit_flanks else flanks)
    rb = B.lib().gf_packed_read_bytes(L)
    lib_defs = [("short-insert", 300, 30, 0, (reads or dreads) // 2 * 2, 1)] + ([("mate-pair", 5000, 500, 1, mp_reads // 2 * 2, 0)] if mp_reads else [])
    libs = []
    for name, is_mean, is_sd, lib_no, n, pull in lib_defs:
        d_reads = torch.empty(n * rb + 64, dtype=torch.uint8, device="cuda")
        d_recs = torch.empty(max(1, n) * 32, dtype=torch.uint8, device="cuda")
        gf.synth_pairs_dev(synth_cfg(is_mean, is_sd, lib_no), 0, n // 2, d_reads.data_ptr(), d_recs.data_ptr())
        libs.append((name, is_mean, is_sd, n, d_reads, d_recs, pull))
    gf.sync()

    def truth(g):
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        return GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11)

    def pipeline(**flags):
        pipe = Pipeline(gf, len(gaps), L, kk, **flags)
        for name, is_mean, is_sd, n, d_reads, d_recs, pull in libs:
            pipe.add_library(DeviceLibrary(name, is_mean, is_sd, n, d_reads, d_recs, pull_mates=pull))
        return pipe
    return types.SimpleNamespace(gf=gf, cfg=cfg, gaps=gaps, kk=kk, gap_len=glen, reads=libs[0][3], libs=libs, truth=truth, pipeline=pipeline)


def timed_steps(pipe, steps):
    """prepare(), a warm-up step, then `steps` steps between barriers: wall milliseconds per step."""
    pipe.prepare()
    pipe.step(1)
    pipe.barrier()
    t0 = time.perf_counter()
    pipe.step(steps)
    pipe.barrier()
    return (time.perf_counter() - t0) * 1e3 / steps


def release():
    """Between two settings of a script, after the caller dropped its Pipeline: the device memory goes back before the next one sizes."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def round_arguments(ap, reps=False, placing=False):
    """The options of a script of an after-pick round; reps: the off / on windows in turn; placing: the placement rule's as well."""
    import bench
    ap.add_argument("--config", default="C4", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    if reps:
        ap.add_argument("--reps", type=int, default=3, help="timed windows per setting, off and on in turn")
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--mp-reads", type=int, default=0, help="read records of the preset's mate-pair library (default: none)")
    ap.add_argument("--gap-len", type=int, default=0)
    ap.add_argument("--anchor-mode", default="exact")
    ap.add_argument("--asm-tiebreak", default="counts", choices=["counts", "none"])
    ap.add_argument("--merge-in-step", action="store_true")
    ap.add_argument("--out", default="")
    if placing:
        ap.add_argument("--seed", type=int, default=16)
        ap.add_argument("--max-mismatch", type=int, default=4)
        ap.add_argument("--min-overlap", type=int, default=48)


def round_setup(args, **flags):
    """(preset_setup's namespace, the Pipeline flags of both settings, the head of the output object) for round_arguments' options."""
    s = preset_setup(args.config, reads=args.reads, gap_len=args.gap_len, mp_reads=args.mp_reads)
    s.gf.set_option("asm_tiebreak", 0 if args.asm_tiebreak == "none" else 1)
    flags = dict(dict(anchor_mode=args.anchor_mode, merge_in_step=args.merge_in_step), **flags)
    return s, flags, {"config": args.config, "gaps": len(s.gaps), "gap_len": s.gap_len, "reads": s.reads, "mp_reads": args.mp_reads,
                      "asm_tiebreak": args.asm_tiebreak}


def spread(ms):
    import numpy as np
    return {"ms": [round(x, 3) for x in ms], "median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def in_turn(s, flags, settings, steps, reps):
    """The step under several settings ({name: Pipeline keywords}): a prepared pipeline each, a warm-up step each, then `reps` windows of
    `steps` steps each, in turn.  Returns ({name: pipeline}, {"ms_per_step_<name>": spread})."""
    pipes = {name: s.pipeline(**kw, **flags) for name, kw in settings.items()}
    for pipe in pipes.values():
        pipe.prepare()
        pipe.step(1)
        pipe.barrier()
    ms = {name: [] for name in pipes}
    for _ in range(reps):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.step(steps)
            pipe.barrier()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return pipes, {"ms_per_step_" + name: spread(v) for name, v in ms.items()}


def off_and_on(s, flags, on, steps, reps):
    """The step with the round off and on (Pipeline keywords `on`): in_turn's protocol.  Returns (the pipeline with the round on,
    {"ms_per_step_off": spread, "ms_per_step_on": spread})."""
    pipes, ms = in_turn(s, flags, {"off": {}, "on": on}, steps, reps)
    return pipes["on"], ms


def round_ms(pipe, gf, enqueue, kernel, steps, reps=1):
    """The round's own time: its launches repeated on the step's results — `reps` windows of `steps` calls, milliseconds per call — and
    the library's launch timer for `kernel`, milliseconds per launch."""
    import torch
    out = []
    gf.timing(True)
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            enqueue()
        e1.record()
        pipe.barrier()
        out.append(e0.elapsed_time(e1) / steps)
    t_ms, n = gf.kernel_time(kernel)
    gf.timing(False)
    return out, round(t_ms / max(1, n), 4)


def emit(out, path):
    text = json.dumps(out)
    print(text, flush=True)
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
