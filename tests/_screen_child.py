"""What test_gpu_screen.py runs in a child process per setting of SCFQ_SCREEN_TABLE_BITS / SCFQ_SCREEN_PREFILTER / SCFQ_SCREEN_PREFILTER_KB:
the fixture's references and pairs through the library, everything it returns as one JSON line.

    python tests/_screen_child.py
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "seq-collection_amd", "pyhost"))
sys.path.insert(0, HERE)

import scfq                                    # noqa: E402
from _screen_check import REF_FIELDS, stats_dict      # noqa: E402

SCREEN = os.path.join(HERE, "golden", "screen")


def main():
    t0 = time.perf_counter()
    paths = [os.path.join(SCREEN, n + ".fa") for n in ("spike", "vector", "rrna")]
    try:
        index = scfq.screen_index_files(paths)
    except scfq.ScfqError as e:
        print(json.dumps(dict(rc=e.rc, text=str(e), seconds=round(time.perf_counter() - t0, 3))))
        return 0
    r1, r2 = (open(os.path.join(SCREEN, f), "rb").read() for f in ("r1.fq", "r2.fq"))
    opts = scfq.screen_opts(min_hits=3)
    s, o1, o2 = scfq.screen_host(index, r1, r2, opts)
    recs = (scfq.ScreenRec * int(s.reads_in))()
    s2 = scfq.screen_file(index, os.path.join(SCREEN, "r1.fq"), os.path.join(SCREEN, "r2.fq"), opts, recs=recs)
    assert stats_dict(s) == stats_dict(s2)
    summary = dict(distinct=int(index.summary.distinct), slots=int(index.summary.slots),
                   refs=[[int(getattr(index.summary.ref[r], f)) for f in REF_FIELDS] for r in range(3)])
    print(json.dumps(dict(rc=0, stats=stats_dict(s), out1=hashlib.sha256(o1).hexdigest(), out2=hashlib.sha256(o2).hexdigest(),
                          recs=[[x.kmers, x.hit_kmers, x.best_hits, x.mask, x.best, x.reserved] for x in recs], summary=summary)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
