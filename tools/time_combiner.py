"""Times AudioCombiner's GPU path on the corpus of tests/test_gpu_combiner.py::test_realistic_corpus_all_vs_all
(64 recordings of 60-180 s, Mel hashprints of synthetic music): the index build (hpfw_gpu_combiner_add), find and
align (k = 8) all-vs-all with self-exclusion, and the Python restatement of combiner.h:100-132 on a few queries.
Prints the hash skew and the events-per-query histogram (what decides whether chunking matters) and one JSON line.

    python tools/time_combiner.py [--reps 5] [--ref-queries 3]

Times are host wall clock around the host-buffer entry points, which end in a device synchronise (they include the
copies of the queries and results); median of --reps after one warm-up call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hpfw_amd  # noqa: E402
from combiner_ref import RefIndex, events_per_query, mel_corpus  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.max(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-queries", type=int, default=3)
    args = ap.parse_args()

    g = hpfw_amd.Gpu(0)
    t0 = time.perf_counter()
    recs = mel_corpus(g)
    t_corpus = time.perf_counter() - t0
    n = [r.size for r in recs]
    allv = np.concatenate(recs)
    counts = np.bincount(allv, minlength=65536)
    top = np.argsort(counts)[::-1][:5]
    print(f"corpus: {len(recs)} recordings, {allv.size} hashprints ({min(n)}..{max(n)} per recording), built in {t_corpus:.1f} s")
    print(f"distinct values {int((counts > 0).sum())}; most frequent: " +
          ", ".join(f"0x{int(v):04x} {counts[v] / allv.size:.2%}" for v in top))

    def build():
        g.combiner_clear()
        g.combiner_add(recs)

    ex = list(range(len(recs)))
    t_build = timed(build, args.reps)
    t_find = timed(lambda: g.combiner_find(recs, ex), args.reps)
    t_align = timed(lambda: g.combiner_align(recs, 8, ex), args.reps)
    ev = np.array(events_per_query(recs, recs, ex))
    edges = [0, 1e5, 2e5, 5e5, 1e6, 2e6, 5e6, 1e7, 1e12]
    hist, _ = np.histogram(ev, bins=edges)
    print("events per query: min %d median %d max %d total %d" % (ev.min(), np.median(ev), ev.max(), ev.sum()))
    for a, b, h in zip(edges[:-1], edges[1:], hist):
        if h:
            print(f"  [{a:.0e}, {b:.0e}): {h}")
    print(f"index build (64 recordings): median {t_build[0]:.2f} ms (min {t_build[1]:.2f}, max {t_build[2]:.2f})")
    print(f"find all-vs-all (64 queries): median {t_find[0]:.2f} ms (min {t_find[1]:.2f}, max {t_find[2]:.2f}); "
          f"{ev.sum() / t_find[0] / 1e3:.1f} M events/s")
    print(f"align all-vs-all, k = 8: median {t_align[0]:.2f} ms (min {t_align[1]:.2f}, max {t_align[2]:.2f})")

    ref = RefIndex(recs)
    qs = list(np.argsort(ev)[:: max(1, len(ev) // max(args.ref_queries, 1))][:args.ref_queries])
    t_ref = []
    got = g.combiner_find([recs[q] for q in qs], [int(q) for q in qs])
    for i, q in enumerate(qs):
        t0 = time.perf_counter()
        r = ref.find(recs[q], int(q))
        t_ref.append(time.perf_counter() - t0)
        same = r == (int(got[i]["rec"]), int(got[i]["cnt"]), int(got[i]["confidence"]), int(got[i]["offset"]))
        print(f"restatement, query {q} ({ev[q]} events): {t_ref[-1] * 1e3:.0f} ms, equal to the GPU: {same}")
    g.close()
    print(json.dumps({"recordings": len(recs), "hashprints": int(allv.size), "events_total": int(ev.sum()),
                      "events_median": int(np.median(ev)), "events_max": int(ev.max()),
                      "build_ms": round(t_build[0], 3), "find_ms": round(t_find[0], 3), "align_ms": round(t_align[0], 3),
                      "ref_ms_per_query": [round(t * 1e3, 1) for t in t_ref],
                      "ref_events": [int(ev[q]) for q in qs]}))


if __name__ == "__main__":
    main()
