#!/usr/bin/env python3
"""Reduce the per-launch phase tables (VOFOD_LDS_PROF_JSON) of 256-frame launches to one table: per phase the mean over launches
of the frames' mean / median / p90 / max, alone and in the pipeline.  usage: phase_summary.py alone.jsonl pipe.jsonl"""
import json
import sys


def reduce(path, frames=256, skip=2):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    rows = [r for r in rows if r["frames"] == frames][skip:]
    if not rows:
        return None
    out = {"launches": len(rows), "span_us": round(sum(r["span_us"] for r in rows) / len(rows), 1)}
    for k in ("start_us", "end_us"):
        out[k] = {q: round(sum(r[k][q] for r in rows) / len(rows), 1) for q in rows[0][k]}
    out["phases"] = {}
    for ph in rows[0]["phases"]:
        out["phases"][ph] = {q: round(sum(r["phases"][ph][q] for r in rows) / len(rows), 2) for q in ("mean", "median", "p90", "max")}
    wv = [r for r in rows if "input_waves" in r]
    if wv:  # the input pass wave by wave: the mean and the last wave's end (us from the frame's start), per cent of the loop spent waiting for loads
        out["input_waves"] = {k: {q: round(sum(r["input_waves"][k][q] for r in wv) / len(wv), 2) for q in ("mean", "median", "p90", "max")} for k in wv[0]["input_waves"]}
    pf = [r["pure_far"] for r in rows if "pure_far" in r]
    if pf:  # lengths of the frames' pure-far lists, and frames per launch whose list is beyond the lean ranks' threshold
        out["pure_far"] = {"bricks": {q: round(sum(r["bricks"][q] for r in pf) / len(pf), 1) for q in ("mean", "median", "p90", "max")},
                           **{k: round(sum(r[k] for r in pf) / len(pf), 1) for k in ("min", "p10", "over_lean_ranks_max")}}
    lc = [r["lean_count"] for r in rows if "lean_count" in r]
    if lc:  # lean count: entries of the frames' code lists and voxels with a counter (mean over launches; the maxima over all launches size the
        # caps), and frames per launch that counted from the list / walked every code / had a list beyond the cap
        out["lean_count"] = {**{k: {**{q: round(sum(r[k][q] for r in lc) / len(lc), 1) for q in ("mean", "median", "p90", "max")}, "max_of_launches": max(r[k]["max"] for r in lc)}
                                for k in ("entries", "counters")},
                             **{k: round(sum(r[k] for r in lc) / len(lc), 1) for k in ("from_list", "walked", "over_lean_count_max")}}
    tl = [r for r in rows if "tail" in r]
    if tl:  # k_tail_far's own stamps for the same frames (one wave per frame)
        out["k_tail_far"] = {ph: {q: round(sum(r["tail"][ph][q] for r in tl) / len(tl), 2) for q in ("mean", "median", "p90", "max")} for ph in tl[0]["tail"]}
    return out


res = {"_note": "k_frame_lds_far, 256 x OS1-128 @ 0.25 m: us per phase from the 100 MHz stamps of every frame's workgroup (tools/phase_table.sh); "
                "alone = one batch at a time; pipeline = four batches in flight (k_key1 of the next batch and the tail of the previous one beside it)",
       "alone": reduce(sys.argv[1]), "pipeline": reduce(sys.argv[2])}
print(json.dumps(res, indent=1))
