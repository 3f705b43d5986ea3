"""Child process of tests/test_gpu_cover_seams.py: GTX_WEIGHTED_FAST is read once per process, so the weighted coverage through the
general per-chunk code runs here.  argv: cases.npz (packed by pack_cases() of the test) and the .npy to write: one coverage row per
weight vector, the cases' regions side by side."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "ibm-cbc-genomic-tools_amd")]


def main(src, dst):
    assert os.environ.get("GTX_WEIGHTED_FAST") == "0"
    import gtx
    z = np.load(src)
    refs, reads, w, roff, qoff, ncls, flags = (z[k] for k in ("refs", "reads", "weights", "refs_off", "reads_off", "n_classes", "flags"))
    out = np.zeros((w.shape[0], len(refs)), dtype=np.uint64)
    e = gtx.Engine(0)
    for i in range(len(ncls)):
        r, q = refs[roff[i]:roff[i + 1]], reads[qoff[i]:qoff[i + 1]]
        e.set_refs(r, int(ncls[i]))
        for v in range(w.shape[0]):
            out[v, roff[i]:roff[i + 1]], _ = e.coverage(q, w[v, qoff[i]:qoff[i + 1]], int(flags[i]))
    e.close()
    np.save(dst, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
