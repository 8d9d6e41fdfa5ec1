"""How many extraction launch sequences are in flight, survey by survey, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 6 --warmup 2
    python scripts/sequences_in_flight.py DIR/*/*_kernel_trace.csv [--chunks-per-survey 10]

A sequence is what one extraction driver thread launches for one chunk: from its `resize_area_lds_kernel` to the last
`feat_*` kernel before the thread's next `resize_area_lds_kernel`.  It is in flight between the start of the first and
the end of the last of these kernels.  Chunks are handed out in survey order, so consecutive groups of
`--chunks-per-survey` chunks (by start time) are the surveys; a survey's period runs from its first chunk's start to the
next survey's first chunk's start.  Printed per survey: the time with 4 / 3 / 2 / 1 / 0 sequences in flight, the time
no extraction kernel runs at all, the window without an extraction kernel that ends with the survey's first kernel
(the hand-over from the survey before), and, once, the hardware queue(s) and stream(s) each driver thread's dispatches
went to and what every hardware queue of the process carried.
"""
import argparse
import csv
from collections import defaultdict


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Thread_Id", "0"),
                         r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
    rows.sort()
    return rows


def chunks_of(rows):
    """[(start, end, thread, [kernel intervals])] per chunk, and thread -> (queues, streams)"""
    by_thread = defaultdict(list)
    for r in rows:
        by_thread[r[3]].append(r)
    chunks, where = [], {}
    for th, rs in by_thread.items():
        if not any("resize_area_lds_kernel" in r[2] for r in rs):
            continue
        where[th] = (sorted({r[4] for r in rs}), sorted({r[5] for r in rs}))
        cur = None
        for r in rs:
            if "resize_area_lds_kernel" in r[2]:
                if cur:
                    chunks.append(cur)
                cur = [r[0], r[1], th, [(r[0], r[1])], r[1]]
            elif cur:
                cur[3].append((r[0], r[1]))
                if "feat_" in r[2]:
                    cur[4] = max(cur[4], r[1])
        if cur:
            chunks.append(cur)
    out = []
    for c in chunks:
        iv = [k for k in c[3] if k[1] <= c[4]]   # nothing after the chunk's last feat_* kernel belongs to it
        out.append((c[0], c[4], c[2], iv))
    out.sort()
    return out, where


def union(intervals):
    merged = []
    for s, e in sorted(intervals):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return merged


def covered(merged, lo, hi):
    return sum(max(0, min(e, hi) - max(s, lo)) for s, e in merged)


def depth_times(chunks, lo, hi, top):
    """time within [lo, hi) at every depth of overlapping chunk intervals"""
    ev = []
    for s, e, _, _ in chunks:
        s, e = max(s, lo), min(e, hi)
        if e > s:
            ev += [(s, 1), (e, -1)]
    ev.sort()
    t, depth, out = lo, 0, [0] * (top + 1)
    for x, d in ev:
        out[min(depth, top)] += x - t
        t, depth = x, depth + d
    out[min(depth, top)] += hi - t
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--chunks-per-survey", type=int, default=10)
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--skip", type=int, default=2, help="surveys left out of the mean (bench.py's warm-up steps; the one "
                    "after them starts behind the barrier between warm-up and timed region)")
    a = ap.parse_args()
    rows = load(a.trace)
    chunks, where = chunks_of(rows)
    n = a.chunks_per_survey
    surveys = [chunks[i:i + n] for i in range(0, len(chunks), n)]
    kernels = union([k for c in chunks for k in c[3]])
    print(f"{len(rows)} dispatches, {len(chunks)} extraction chunks on {len(where)} driver threads, "
          f"{len(surveys)} surveys of {n} chunks")
    ms = 1e-6
    head = " ".join(f"{k}_in_flight" for k in range(a.sequences, -1, -1))
    print(f"survey period_ms {head} no_extract_kernel_ms handover_window_ms chunk_ms_median drivers")
    for i, sv in enumerate(surveys):
        lo = sv[0][0]
        last = i + 1 == len(surveys)
        hi = max(c[1] for c in sv) if last else surveys[i + 1][0][0]
        d = depth_times(chunks, lo, hi, a.sequences)
        idle = (hi - lo) - covered(kernels, lo, hi)
        before = max((e for s, e in kernels if s < lo), default=lo)
        window = max(0, lo - before)
        lens = sorted(c[1] - c[0] for c in sv)
        print(f"{i:6d} {(hi - lo) * ms:9.2f} " + " ".join(f"{d[k] * ms:11.2f}" for k in range(a.sequences, -1, -1)) +
              f" {idle * ms:20.2f} {window * ms:18.2f} {lens[len(lens) // 2] * ms:15.2f} {len({c[2] for c in sv}):7d}"
              + ("  (last survey: to its last kernel)" if last else ""))
    full = list(range(a.skip, len(surveys) - 1))   # whole periods of the timed region (the last survey has no successor)
    if full:
        tot = [0] * (a.sequences + 1)
        period = idle = window = 0
        for i in full:
            lo, hi = surveys[i][0][0], surveys[i + 1][0][0]
            for k, v in enumerate(depth_times(chunks, lo, hi, a.sequences)):
                tot[k] += v
            period += hi - lo
            idle += (hi - lo) - covered(kernels, lo, hi)
            nxt = surveys[i + 1][0][0]
            window += max(0, nxt - max((e for s, e in kernels if s < nxt), default=nxt))
        m = len(full)
        print(f"mean over surveys {full[0]}..{full[-1]}: period {period * ms / m:.2f} ms; " +
              ", ".join(f"{k} in flight {tot[k] * ms / m:.2f} ms" for k in range(a.sequences, -1, -1)) +
              f"; fewer than {a.sequences}: {sum(tot[:a.sequences]) * ms / m:.2f} ms "
              f"({100.0 * sum(tot[:a.sequences]) / max(period, 1):.1f} % of the period); no extraction kernel "
              f"{idle * ms / m:.2f} ms, of it the window at the hand-over to the next survey {window * ms / m:.2f} ms")
    print("driver thread -> hardware queue(s), stream(s) of its dispatches:")
    seen = defaultdict(int)
    for th, (q, s) in where.items():
        seen[(tuple(q), tuple(s))] += 1
    for (q, s), cnt in sorted(seen.items()):
        print(f"  queue {','.join(q)}  stream {','.join(s)}  : {cnt} driver threads")
    queues = defaultdict(set)
    for th, (q, s) in where.items():
        for x in q:
            queues[x].update(s)
    shared = {q: sorted(s) for q, s in queues.items() if len(s) > 1}
    print("hardware queues that carry more than one extraction stream:", shared if shared else "none")
    print("every hardware queue of the process: dispatches, streams, the kernel it ran longest")
    per_queue = defaultdict(lambda: [0, set(), defaultdict(int)])
    for s, e, name, _, q, st in rows:
        pq = per_queue[q]
        pq[0] += 1
        pq[1].add(st)
        pq[2][name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:40]] += e - s
    for q, (cnt, sts, names) in sorted(per_queue.items()):
        top = max(names.items(), key=lambda kv: kv[1])
        ext = sorted(x for x in sts if any(x in w[1] for w in where.values()))
        print(f"  queue {q}: {cnt} dispatches on {len(sts)} streams (extraction streams: {','.join(ext) or 'none'}); "
              f"{top[0]} {top[1] * ms:.1f} ms")


if __name__ == "__main__":
    main()
