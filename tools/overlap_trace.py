"""The forked eval step in a kernel trace: python tools/overlap_trace.py KERNEL_TRACE.csv [STEPS]

Reads the kernel trace of `rocprofv3 --kernel-trace --stats -- python bench.py --train-steps 0 --no-cpu-baseline --no-hbm-kernels`
and prints one JSON object:
  us_per_step     total duration by kernel family over all steps of the pass (warm-up included), divided by their number
  steps           per timed step, in us from the step's k_rgb_to_ycc: the interval of the level-0 k_plc_wino and k_cgp16 launches,
                  the interval and busy time of the kernels on the other stream (the tail chain), and what the main stream waited
                  for at the join: the gap between its last kernel before the join and its first one after, against the end of the tail
A step is what lies between two k_rgb_to_ycc launches; the main stream is the one of that launch."""
import csv
import json
import re
import sys


def family(name):
    n = re.sub(r"^void\s+", "", name).replace("(anonymous namespace)::", "")
    n = re.sub(r"\(.*$", "", n)
    n = re.sub(r"<.*$", "", n)
    return n.replace("lldwt::", "").strip()


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    skey = "Stream_Id" if "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows}) > 1 else "Queue_Id"
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), family(r["Kernel_Name"]), r[skey]) for r in rows))
    marks = [i for i, k in enumerate(ks) if k[2] == "k_rgb_to_ycc"]
    nsteps = len(marks)
    fam = {}
    for s, e, f, _ in ks[marks[0]:]:
        fam[f] = fam.get(f, 0.0) + (e - s) / 1e3
    top = sorted(fam.items(), key=lambda kv: -kv[1])
    out = {"stream_key": skey, "steps_in_pass": nsteps,
           "us_per_step": dict([(f, round(v / nsteps, 1)) for f, v in top[:9]] + [("all kernels", round(sum(fam.values()) / nsteps, 1))]),
           "steps": []}
    want = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for a, b in list(zip(marks, marks[1:] + [len(ks)]))[-want:]:
        step = ks[a:b]
        t0, main = step[0][0], step[0][3]
        us = lambda t: round((t - t0) / 1e3, 1)
        plc = max((k for k in step if k[2] == "k_plc_wino"), key=lambda k: k[1] - k[0])
        cgp = max((k for k in step if k[2] == "k_cgp16"), key=lambda k: k[1] - k[0])
        tail = [k for k in step if k[3] != main]
        d = {"wall_us": us(max(k[1] for k in step)), "plc0": [us(plc[0]), us(plc[1])], "cgp0": [us(cgp[0]), us(cgp[1])],
             "lift_main_us": round(sum(k[1] - k[0] for k in step if k[2] == "k_lift_fused_f16" and k[3] == main) / 1e3, 1)}
        if tail:
            t_end = max(k[1] for k in tail)
            before = max((k for k in step if k[3] == main and k[1] <= max(t_end, cgp[1]) and k[0] < t_end), key=lambda k: k[1])
            after = min((k for k in step if k[3] == main and k[0] >= max(t_end, before[1])), key=lambda k: k[0], default=None)
            d.update({"tail": [us(min(k[0] for k in tail)), us(t_end)], "tail_kernels": len(tail),
                      "tail_busy_us": round(sum(k[1] - k[0] for k in tail) / 1e3, 1),
                      "tail_lift_us": round(sum(k[1] - k[0] for k in tail if k[2] == "k_lift_fused_f16") / 1e3, 1),
                      "main_last_before_join": [before[2], us(before[1])],
                      "main_first_after_join": [after[2], us(after[0])] if after else None,
                      "join_wait_us": round((after[0] - before[1]) / 1e3, 1) if after else None})
        out["steps"].append(d)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
