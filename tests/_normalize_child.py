"""What test_gpu_normalize.py runs in a child process per setting of SCFQ_NORM_LDS_WINDOWS / SCFQ_KCOUNT_START_BITS (both are read once
per process):

    python tests/_normalize_child.py cases NAME [LDS_WINDOWS]   a case set of _normalize_cases.py, compared with the checker in the child
    python tests/_normalize_child.py fixture [TABLE_BITS]       the fixture's pairs through the two-pass form, what it returns as JSON

One JSON line on stdout either way."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "seq-collection_amd", "pyhost"))
sys.path.insert(0, HERE)

import scfq                                    # noqa: E402
from _normalize_check import stats_dict      # noqa: E402

NORM = os.path.join(HERE, "golden", "normalize")


def fixture(table_bits):
    r1, r2 = (open(os.path.join(NORM, f), "rb").read() for f in ("r1.fq", "r2.fq"))
    opts = scfq.norm_opts(k=21, canonical=True, table_bits=table_bits, target=20, min_depth=3)
    try:
        s, hist, o1, o2 = scfq.norm_host(None, r1, r2, opts, bins=1002)
    except scfq.ScfqError as e:
        return dict(rc=e.rc, text=str(e))
    recs = (scfq.NormRec * int(s.reads_in))()
    s2, hist2 = scfq.norm_file(None, os.path.join(NORM, "r1.fq"), os.path.join(NORM, "r2.fq.gz"), opts, recs=recs, bins=1002)
    assert stats_dict(s) == stats_dict(s2) and hist.tolist() == hist2.tolist()
    return dict(rc=0, stats=stats_dict(s), slots=int(s.slots), passes=int(s.passes), out1=hashlib.sha256(o1).hexdigest(), out2=hashlib.sha256(o2).hexdigest(),
                hist=hist.tolist(), recs=[[x.kmers, x.depth, x.min_count, x.weak] for x in recs])


def main(argv):
    if argv[1] == "fixture":
        print(json.dumps(fixture(int(argv[2]) if len(argv) > 2 else 0)))
        return 0
    import torch
    from _normalize_cases import CASES
    assert torch.cuda.is_available()
    scfq.set_wait_stream(torch.cuda.current_stream().cuda_stream)
    args = [int(argv[3])] if len(argv) > 3 else []
    print(json.dumps(dict(rc=0, case=argv[2], calls=CASES[argv[2]](torch, scfq, *args))))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
