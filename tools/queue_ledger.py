#!/usr/bin/env python3
"""Where a hardware queue's time goes, from one rocprofv3 --kernel-trace run of the flagship workload.

    rocprofv3 --kernel-trace -d DIR --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/queue_ledger.py DIR [--steps 20] [--occupancy FILE]

Kernels that share a hardware queue run one after the other, so per queue the kernel records tile the time line:
what is under no record is time in which the queue ran nothing. Per queue the window is the last `steps` /
(`steps` + warm-up) of its decoder launches (the timed region of bench.py: every step puts the same number of launches
on a queue), from the start of the first kernel in it to the end of the last; the run's window is from the earliest of
those starts to the latest of those ends (bench.py synchronises before and after the timed steps, not between them).
A queue's nothing is what lies between its kernels plus what lies between its own window and the run's: the time in
which it had run out of work while another queue still had some -- streams unevenly spread over the queues.

Prints, per queue and in total: time under decode_fused_kernel, under encode_*, under anything else, under nothing;
the nothing split by (previous kernel -> next kernel) with count, mean, p50, p90; and, with --occupancy (the output of
tools/occupancy_trace.py, whose workgroups log their own begin and end), a decoder launch's length against its mean
workgroup's span -- the launch's ramp and tail.
"""
import argparse
import collections
import csv
import glob
import os
import re
import sys


def kind(name):
    if "decode_fused_kernel" in name:
        return "dec"
    if "encode_" in name:
        return "enc"
    return "other"


def pct(v, q):
    if not v:
        return 0.0
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def load(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            sys.exit(f"queue_ledger: no *kernel_trace.csv under {path}")
        path = max(found, key=os.path.getsize)  # (a child process that launched nothing leaves a small one)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            q = r.get("Queue_Id", r.get("Queue_ID", "0"))
            rows.append((q, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind(r["Kernel_Name"]), r["Kernel_Name"],
                         r.get("Stream_Id", "?")))
    return path, rows


def ledger(rows, steps, warmup):
    by_q = collections.defaultdict(list)
    recs_st = collections.defaultdict(list)
    for q, s, e, k, _, st in rows:
        by_q[q].append((s, e, k))
        recs_st[q].append((s, e, k, st))
    out = {}
    for q, recs in by_q.items():
        recs.sort()
        dec_starts = [s for s, _, k in recs if k == "dec"]
        if len(dec_starts) < 8:
            continue  # (a queue the runtime used for copies or a handful of set-up kernels)
        # the timed steps: the last steps / (steps + warmup) of the queue's decoder launches
        first = dec_starts[len(dec_starts) - (len(dec_starts) * steps) // (steps + warmup)]
        # ... from the encoder in front of that decoder, if it is there
        i0 = next(i for i, r in enumerate(recs) if r[0] == first)
        if i0 and recs[i0 - 1][2] == "enc":
            i0 -= 1
        win = recs[i0:]
        t = {"dec": 0, "enc": 0, "other": 0, "idle": 0, "overlap": 0}
        gaps = collections.defaultdict(list)
        n = collections.Counter()
        prev_end, prev_kind = None, None
        for s, e, k in win:
            n[k] += 1
            if prev_end is not None:
                g = s - prev_end
                if g >= 0:
                    t["idle"] += g
                    key = f"{prev_kind}->{k}" if (prev_kind, k) in (("enc", "dec"), ("dec", "enc")) else "other"
                    gaps[key].append(g)
                else:
                    t["overlap"] += -g
            t[k] += e - s
            prev_end, prev_kind = max(e, prev_end or e), k
        out[q] = {"span": win[-1][1] - win[0][0], "t0": win[0][0], "t1": win[-1][1], "t": t, "gaps": gaps, "n": n,
                  "streams": len({st for s_, _, k, st in recs_st[q] if k == "dec" and s_ >= win[0][0]}),
                  "dec_len": [e - s for s, e, k in win if k == "dec"], "enc_len": [e - s for s, e, k in win if k == "enc"]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="rocprofv3 output directory, or the *_kernel_trace.csv itself")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-tokens", type=int, default=256 * 48, help="target tokens per batch (flagship: 256 x 48)")
    ap.add_argument("--occupancy", help="output of tools/occupancy_trace.py on the same library (decoder workgroup spans)")
    a = ap.parse_args()
    path, rows = load(a.trace)
    led = ledger(rows, a.steps, a.warmup)
    names = collections.Counter(r[4] for r in rows)
    print(f"# {os.path.basename(path)}: {len(rows)} kernel records on {len(set(r[0] for r in rows))} queue ids, "
          f"{len(led)} with decoder launches; window = the last {a.steps}/{a.steps + a.warmup} of each queue's decoders")
    for nm, c in names.most_common(6):
        print(f"#   {c:6d} x {nm[:150]}")
    if not led:
        sys.exit("queue_ledger: no queue with decoder launches in the trace")
    T0, T1 = min(L["t0"] for L in led.values()), max(L["t1"] for L in led.values())
    run = T1 - T0
    tot = collections.Counter()
    tot_gaps = collections.defaultdict(list)
    dec_len, enc_len, pairs = [], [], 0
    print(f"\n## per queue (ms; the run's window is {run/1e6:.2f} ms; 'between' = no kernel record between two of the queue's "
          f"kernels, 'drained' = the queue's own window against the run's)")
    print(f"{'queue':>6} {'streams':>7} {'batches':>7} {'own span':>9} {'decoder':>9} {'encoder':>9} {'other':>7} {'between':>8} {'drained':>8} {'nothing %':>9}")
    for q in sorted(led, key=str):
        L = led[q]
        t = L["t"]
        drained = run - L["span"]
        print(f"{q:>6} {L['streams']:7d} {L['n']['dec']:7d} {L['span']/1e6:9.2f} {t['dec']/1e6:9.2f} {t['enc']/1e6:9.2f} {t['other']/1e6:7.3f} "
              f"{t['idle']/1e6:8.2f} {drained/1e6:8.2f} {100.0*(t['idle'] + drained)/run:8.1f}%"
              + (f"  (records overlap by {t['overlap']/1e3:.1f} us)" if t["overlap"] else ""))
        tot.update(t)
        tot["drained"] += drained
        pairs += L["n"]["dec"]
        dec_len += L["dec_len"]
        enc_len += L["enc_len"]
        for k, v in L["gaps"].items():
            tot_gaps[k] += v
    nq = len(led)
    nb = max(1, pairs)
    print(f"{'all':>6} {sum(L['streams'] for L in led.values()):7d} {pairs:7d} {'':>9} {tot['dec']/1e6:9.2f} {tot['enc']/1e6:9.2f} {tot['other']/1e6:7.3f} "
          f"{tot['idle']/1e6:8.2f} {tot['drained']/1e6:8.2f} {100.0*(tot['idle'] + tot['drained'])/(nq*run):8.1f}%")
    per = nq * run / nb
    print(f"\nper batch and queue ({nq} queues x {run/1e6:.2f} ms / {pairs} batches): {per/1e3:.0f} us = decoder {tot['dec']/nb/1e3:.0f} "
          f"+ encoder {tot['enc']/nb/1e3:.0f} + other {tot['other']/nb/1e3:.1f} + nothing {(tot['idle'] + tot['drained'])/nb/1e3:.0f} "
          f"(between kernels {tot['idle']/nb/1e3:.0f}, drained {tot['drained']/nb/1e3:.0f})")
    print(f"rate the window implies: {pairs} batches x {a.batch_tokens} tokens / {run/1e6:.2f} ms = "
          f"{pairs*a.batch_tokens/(run/1e3):.2f} M tok/s (under the tracer); with the batches spread evenly over the queues and "
          f"nothing else changed: {nq*a.batch_tokens/((tot['dec'] + tot['enc'] + tot['other'] + tot['idle'])/nb/1e3):.2f} M")
    print("\n## nothing, by (previous kernel -> next kernel) on the queue (us)")
    print(f"{'boundary':>10} {'count':>7} {'total ms':>9} {'mean':>8} {'p50':>8} {'p90':>8} {'max':>9}")
    for k in ("enc->dec", "dec->enc", "other"):
        v = tot_gaps.get(k, [])
        if v:
            print(f"{k:>10} {len(v):7d} {sum(v)/1e6:9.2f} {sum(v)/len(v)/1e3:8.1f} {pct(v,0.5)/1e3:8.1f} {pct(v,0.9)/1e3:8.1f} {max(v)/1e3:9.1f}")
        else:
            print(f"{k:>10} {0:7d}")
    print("\n## launch lengths (us)")
    for nm, v in (("decoder", dec_len), ("encoder", enc_len)):
        if v:
            print(f"{nm:>10} {len(v):6d} launches: mean {sum(v)/len(v)/1e3:8.1f}  p10 {pct(v,0.1)/1e3:8.1f}  p50 {pct(v,0.5)/1e3:8.1f}  p90 {pct(v,0.9)/1e3:8.1f}")
    if a.occupancy:
        txt = open(a.occupancy).read()
        m = re.findall(r"decoder workgroups (\d+): mean (\d+(?:\.\d+)?) us, p10 (\d+(?:\.\d+)?), p50 (\d+(?:\.\d+)?), p90 (\d+(?:\.\d+)?)", txt)
        if m and dec_len:
            cnt, mean, p10, p50, p90 = m[-1]
            launch = sum(dec_len) / len(dec_len) / 1e3
            print(f"\n## inside a decoder launch\nfirst workgroup's start to last workgroup's end (the kernel record): {launch:.0f} us; "
                  f"a workgroup's own span (occupancy trace, {cnt} workgroups): mean {mean} us (p10-p90 {p10}-{p90})\n"
                  f"ramp and tail of a launch: {launch - float(mean):.0f} us = {100.0*(launch - float(mean))/launch:.1f} % of it")
        else:
            print("\n## inside a decoder launch: no 'decoder workgroups' line in " + a.occupancy)


if __name__ == "__main__":
    main()
