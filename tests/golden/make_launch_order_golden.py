"""Generates tests/golden/bwd_launch_order.json: the backward's launch order -- every (profiler record name, stream) in host
enqueue order -- for each case of tests/test_bwd_schedule_gpu.py, taken with that module's own trace_case (needs the GPU).

Record it at the commit whose schedules are the reference, i.e. BEFORE a change that must leave them alone, and name that commit:

    python tests/golden/make_launch_order_golden.py --commit <hash of the commit that was built>
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_bwd_schedule_gpu as T      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the library under trace was built from (stored in the file)')
    ap.add_argument('--out', default=T.GOLDEN_JSON)
    a = ap.parse_args()
    cases = {case: T.trace_case(case) for case in T.CASES}
    for case, recs in cases.items():
        print('%-20s %4d launches on %d stream(s)' % (case, len(recs), len({s for _, s in recs})))
    body = ',\n'.join('  %s: [\n%s\n  ]' % (json.dumps(case), ',\n'.join('    ' + json.dumps(r) for r in recs)) for case, recs in cases.items())
    with open(a.out, 'w') as f:
        f.write('{"commit": %s,\n "cases": {\n%s\n }}\n' % (json.dumps(a.commit), body))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
