#!/usr/bin/env python3
"""Summarises the wave-priority screen of the BLAKE3 compression stream
(tools/valu_bank.hip, variants compiled_raw*) and the kernel's counter passes
before / after into the issue model the bench reads.  Cycles per VALU
instruction per SIMD as tools/valu_issue_summary.py reads them (launches where
every SIMD held the same number of waves), one value per repeat of the run.
usage: tools/valu_prio_summary.py SCREEN.jsonl PMC_INSTS_PARENT.json
PMC_CLOCK_PARENT.json PMC_INSTS_NEW.json PMC_CLOCK_NEW.json SCREEN_OUT.json
MODEL_OUT.json"""
import json
import sys

WINNER = "compiled_raw_prio_a"
WHAT = {"compiled_raw": "the kernel's G stream with the compiler's pads, no s_setprio",
        "compiled_raw_prio_a": "priority 1 on the 4-cycle runs, 0 on the 2-cycle runs",
        "compiled_raw_prio_b": "priority 0 on the 4-cycle runs, 1 on the 2-cycle runs",
        "compiled_raw_prio_c": "flips at the runs of 8 only: 0 on the 8-long 2-cycle runs, 1 elsewhere",
        "compiled_raw_prio_static": "no flips: every other wave of a SIMD at priority 1 for the whole loop",
        "compiled_raw_lo": "compiled_raw with its registers packed downwards inside their banks (fits 8 waves)",
        "compiled_raw_prio_a_lo": "compiled_raw_prio_a with its registers packed the same way"}


def screen(path):
    out = {}
    for line in open(path):
        d = json.loads(line)
        h = d["waves_per_simd_hist"]
        if d["variant"] not in WHAT or len(h) != 1:
            continue
        v = out.setdefault(d["variant"], {"what": WHAT[d["variant"]], "cycles_per_valu_instruction": {}})
        v["cycles_per_valu_instruction"].setdefault(str(d["waves_per_simd"]), []).append(
            round(next(iter(h.values()))[1], 3))
    return out


def kernel(insts, clock):
    i, c = json.load(open(insts)), json.load(open(clock))
    cyc = i["counters"]["GRBM_GUI_ACTIVE"] / 8  # 8 XCDs
    return {"kernel": i["kernel"], "valu_wave_instructions": int(i["counters"]["SQ_INSTS_VALU"]),
            "cycles_per_valu_instruction_per_simd": round(cyc * 1024 / i["counters"]["SQ_INSTS_VALU"], 3),
            "clock_ghz": c["clock_ghz"], "dispatch_ms_clock_pass": c["avg_duration_ms_profiled"],
            "dispatch_ms_insts_pass": i["avg_duration_ms_profiled"]}


def main():
    scr, ip, cp, in_, cn, out_s, out_m = sys.argv[1:8]
    s = screen(scr)
    base, win = (s[k]["cycles_per_valu_instruction"]["4"] for k in ("compiled_raw", WINNER))
    res = {"what": "wave-priority variants of the BLAKE3 compression stream, cycles per VALU "
                   "instruction per SIMD by waves per SIMD, one value per repeat in one run "
                   "(tools/valu_bank.hip, 256-thread workgroups); s_setprio and s_nop not counted",
           "variants": s,
           "at_4_waves": {"compiled_raw": base, "winner": WINNER, "winner_cycles": win,
                          "spread_of_compiled_raw_repeats": round(max(base) - min(base), 3)}}
    json.dump(res, open(out_s, "w"), indent=1)
    cpi = sorted(win)[len(win) // 2]
    old, new = kernel(ip, cp), kernel(in_, cn)
    model = {
        "what": "issue cost of the BLAKE3 compression stream with wave priority by run "
                "(csrc/b3_compress.hpp, B3_PRIO 1) and the kernel's own counters on the C2 "
                "bench, before (B3_PRIO 0 build) and after",
        "b3_groups_c2_pmc": new,
        "b3_groups_c2_pmc_parent": old,
        "model": {
            "cycles_per_wave_instruction_mixed_stream": cpi,
            "note": "the G stream with priority 1 on its 4-cycle runs and 0 on its 2-cycle runs, "
                    "4 waves per SIMD; without the flips the same stream costs "
                    f"{sorted(base)[len(base) // 2]} (valu_prio_screen.json).  The ceiling is 1024 "
                    "SIMDs x 64 lanes x clock / that x 680 algorithmic ops / 681 instructions "
                    "per compression",
            "peak_tops_at_2p4ghz": round(1024 * 64 * 2.4e9 / cpi * 680 / 681 / 1e12, 3)}}
    json.dump(model, open(out_m, "w"), indent=1)
    print(json.dumps(res["at_4_waves"]), json.dumps(model["model"]), json.dumps(new), json.dumps(old))


if __name__ == "__main__":
    main()
