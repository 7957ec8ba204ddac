"""The reference's notebook (examples/python/liveid.ipynb) on the GPU path:

    python examples/liveid.py --index originals/*.wav --search slices/*.wav [--dump dump.pkl]
    python examples/liveid.py --index originals/*.wav --timeline concert.wav --min-score 10 [--tempos 0.96 1 1.04]

prepare() -> pickle dump of [(hashprint array, name)] (cells 4-5) -> ten best tracks per query by the
sliding Hamming scan (cell 9, here one batched scan in HBM instead of a process pool over Cython
loops) -> share of queries whose best track is contained in the query's name (cells 11-12).

--timeline FILE (not in the notebook): the set list of one long recording, 5 s windows every 2.5 s, each segment with the
score of its best window.  --min-score has no default: pick it from recordings you know."""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hpfw_amd  # noqa: E402
from hpfw_amd.liveid import LiveSongIdentification  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--index", nargs="*", default=[])
ap.add_argument("--load", help="pickle written by --dump (cell 6)")
ap.add_argument("--dump", help="write prepare()'s result as a pickle (cell 5)")
ap.add_argument("--search", nargs="*", default=[])
ap.add_argument("--cache", default="")
ap.add_argument("--timeline", help="a long recording: print the indexed songs it holds, with times")
ap.add_argument("--min-score", type=float, help="required with --timeline")
ap.add_argument("--shifts", nargs="*", type=int, help="bin shifts to search as well (--timeline)")
ap.add_argument("--tempos", nargs="*", type=float, help="tempo factors to search as well (--timeline)")
ap.add_argument("--min-overlap", type=int, help="--timeline by the overlap rule over at least this many hashprints: song edges "
                                                 "and indexed items shorter than a window (DESIGN.md section 18); not with "
                                                 "--shifts, --tempos or --devices")
ap.add_argument("--devices", nargs="*", type=int, help="shard the index over these devices, one ordinal per shard")
args = ap.parse_args()

liveid = LiveSongIdentification(cache=args.cache, devices=args.devices or None)
if args.load:
    with open(args.load, "rb") as fp:
        hashprints = pickle.load(fp)
else:
    hashprints = liveid.collector.prepare(args.index)
if args.dump:
    with open(args.dump, "wb") as fp:
        pickle.dump(hashprints, fp)
liveid.build(hashprints)
if args.timeline:
    if args.min_score is None:
        ap.error("--timeline needs --min-score")
    for start, end, name, score, offset, shift, tempo in liveid.timeline(args.timeline, args.min_score, shifts=args.shifts or None,
                                                                         tempos=args.tempos or None, min_overlap=args.min_overlap):
        print(f"{start:8.1f} s - {end:8.1f} s  {name}  score {score:.1f}  from {offset:.1f} s  shift {shift}  tempo {tempo:g}")
ans = liveid.top(args.search, 10)
for label, top in ans:
    print("Finding ", label)
    print("   ", [(d, name) for d, name, _ in top] if top else "INVALID QUERY")
right = sum(1 for label, top in ans if top and top[0][1] in label)
print("accuracy", right / max(len(ans), 1))
liveid.close()
