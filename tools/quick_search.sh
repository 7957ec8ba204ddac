#!/bin/bash
# search-only timing: bench.py's search section
cd "$(dirname "$0")/.."
timeout -k 10 600 python bench.py --full --no-cpu-baseline --steps 1 --warmup 1 --clips 64 "$@" 2> >(tail -2 >&2) | python3 -c "
import json,sys
for ln in sys.stdin:
    if ln.startswith('{'):
        d = json.loads(ln)['search']
        print(d['ms_per_search'], '%.4g' % d['value'], d['planted_queries_found'], d.get('scan_kernel'))
"
