"""The songs of a feed that is still running:

    some-decoder ... -f s16le -ac 1 -ar 44100 - | python examples/live_streams.py --index originals/ --min-score 10

    some-capture ... -f s16le -ac 1 -ar 48000 - | python examples/live_streams.py --index originals/ --min-score 10 --rate 48000

Indexes every WAV file of a directory, then reads raw mono PCM16 at --rate (44.1 kHz unless given) from stdin in chunks of 0.5 s
and prints a line when a song starts and when it has ended: 5 s windows every 2.5 s, as LiveSongIdentification.timeline() cuts a
file, but window by window as the samples arrive.  --min-score has no default: pick it from recordings you know.  A feed at
another rate (any integer rate from 8 000 to 192 000 Hz) is converted to 44.1 kHz on the GPU chunk by chunk, exactly as a file
at that rate is; the files of the index may then be at other rates too."""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hpfw_amd.liveid import LiveSongIdentification  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--index", required=True, help="a directory of WAV files (44.1 kHz)")
ap.add_argument("--min-score", type=float, required=True)
ap.add_argument("--shifts", nargs="*", type=int, help="bin shifts to search as well")
ap.add_argument("--tempos", nargs="*", type=float, help="tempo factors to search as well")
ap.add_argument("--rate", type=int, default=44100, help="the feed's sample rate in Hz, 8000 to 192000")
ap.add_argument("--cache", default="")
ap.add_argument("--devices", nargs="*", type=int, help="shard the index over these devices, one ordinal per shard")
args = ap.parse_args()

CHUNK = args.rate // 2                                     # 0.5 s


def line(what, seg):
    start, end, name, score, offset, shift, tempo = seg
    print(f"{what:6s} {start:8.1f} s - {end:8.1f} s  {name}  score {score:.1f}  from {offset:.1f} s  shift {shift}  tempo {tempo:g}",
          flush=True)


liveid = LiveSongIdentification(cache=args.cache, devices=args.devices or None, resample=args.rate != 44100)
liveid.index(sorted(glob.glob(os.path.join(args.index, "*.wav"))))
with liveid.streams(1, args.min_score, shifts=args.shifts or None, tempos=args.tempos or None, rate=args.rate) as live:
    playing = None                                         # (start, name) of the segment last announced
    while True:
        raw = sys.stdin.buffer.read(2 * CHUNK)
        if len(raw) < 2:
            break
        for _, seg in live.push([np.frombuffer(raw[:len(raw) & ~1], "<i2")]):
            line("closed", seg)
        now = live.open()[0]
        if now is not None and (now[0], now[2]) != playing:
            playing = (now[0], now[2])
            line("opened", now)
    tail = np.zeros(live.tail(0), np.int16)                # the feed has ended: its last outputs wait for these
    for _, seg in live.push([tail]) + live.finish():
        line("closed", seg)
liveid.close()
