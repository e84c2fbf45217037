"""tools/queue_ledger.py on a synthetic kernel trace: twenty streams spread 4 / 5 / 5 / 6 over four queues, every batch an
encoder of 250 us and a decoder of 2,400 us with 5 us between kernels; the queues
start the timed steps together, as after the benchmark's synchronise. The ledger must find the streams and batches per
queue, put the queues' early ends under 'drained' and the 5 us under 'between', and name the rate level queues would give."""
import csv
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ledger_splits_gaps_from_drained_queues(tmp_path):
    enc, dec, gap, calls = 250_000, 2_400_000, 5_000, 100  # ns; calls per stream (80 of them in the window: 20 of 25 steps)
    rows, stream = [], 0
    for q, n_streams in enumerate((4, 5, 5, 6), start=1):
        t = 1_000_000
        ids = list(range(stream, stream + n_streams))
        stream += n_streams
        for call in range(calls):
            if call == calls // 5:  # the warm-up ends with a synchronise: the timed steps start together on every queue
                t = 2_000_000_000
            for st in ids:
                for name, d in (("void slimt_hip::encode_tall_kernel<24, 2, 4>(slimt_hip::FusedEncodeArgs)", enc),
                                ("void slimt_hip::decode_fused_kernel<false, 4>(slimt_hip::FusedDecodeArgs)", dec)):
                    rows.append({"Kind": "KERNEL_DISPATCH", "Queue_Id": q, "Stream_Id": st, "Kernel_Name": name,
                                 "Start_Timestamp": t, "End_Timestamp": t + d})
                    t += d + gap
    os.makedirs(tmp_path / "host")
    with open(tmp_path / "host" / "1_kernel_trace.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "queue_ledger.py"), str(tmp_path)],
                         capture_output=True, text=True, check=True).stdout
    per_queue = re.findall(r"^\s+([1-4])\s+(\d+)\s+(\d+)\s", out, flags=re.M)
    assert [(int(q), int(s), int(b)) for q, s, b in per_queue] == [(1, 4, 320), (2, 5, 400), (3, 5, 400), (4, 6, 480)], out
    m = re.search(r"per batch and queue .*: (\d+) us = decoder (\d+) \+ encoder (\d+) \+ other [\d.]+ \+ nothing (\d+) "
                  r"\(between kernels (\d+), drained (\d+)\)", out)
    assert m, out
    total, d, e, nothing, between, drained = (int(x) for x in m.groups())
    # the run lasts as long as the queue with six streams: 6 x 80 batches of 2,660 us on each of 4 queues, 1,600 batches
    assert abs(total - 6 * 80 * 2660 * 4 // 1600) <= 2 and (d, e) == (2400, 250), out
    assert between == 10 and abs(drained - (total - 2660)) <= 2 and nothing == between + drained, out
    level = re.search(r"nothing else changed: ([\d.]+) M", out)
    assert level and abs(float(level.group(1)) - 4 * 12288 / 2660.0) < 0.02, out
