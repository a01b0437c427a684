"""What test_gpu_kcount.py runs in a child process per setting of SCFQ_KCOUNT_START_BITS / SCFQ_KCOUNT_MAX_PROBE / SCFQ_KCOUNT_MERGE (the library
reads them once per process): one or two FASTQ files through scfq_kcount_files, everything the table returns as one JSON line.

    python tests/_kcount_child.py K FLAGS TABLE_BITS IN.fq [IN2.fq]
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "seq-collection_amd", "pyhost"))
sys.path.insert(0, HERE)

import numpy as np                             # noqa: E402
import scfq                                    # noqa: E402
from _kcount_check import SUMMARY_FIELDS       # noqa: E402


def main():
    k, flags, bits = (int(v) for v in sys.argv[1:4])
    paths = sys.argv[4:]
    t0 = time.perf_counter()
    try:
        s, t = scfq.kcount_files(paths[0], paths[1] if len(paths) > 1 else None, k=k, flags=flags, table_bits=bits)
    except scfq.ScfqError as e:
        print(json.dumps(dict(rc=e.rc, text=str(e), handle=e.handle, seconds=round(time.perf_counter() - t0, 3))))
        return 0
    rows = t.dump(1, 0)
    keys = rows[:, 0] if rows.size else np.zeros(0, np.uint64)
    out = dict(rc=0, summary={f: int(getattr(s, f)) for f in SUMMARY_FIELDS}, dump=[[int(a), int(b)] for a, b in rows.tolist()],
               hist=t.hist(int(s.max_count) + 2).tolist(), query=t.query(keys).tolist(), seconds=round(time.perf_counter() - t0, 3))
    t.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
