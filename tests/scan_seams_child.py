"""Child process of tests/test_gpu_scan_seams.py: GTX_SCAN_BUCKETS and GTX_SCAN_FUSED are read once per process, so the partition path
with buckets of several parts, and the device entry with the parts NOT writing the windows, run here.  argv: cases.npz (packed by
pack_cases() of the test: reads in no order) and the .npy to write: one row of windows per weight variant (none, signed), the cases side
by side.  Every case goes through gtx_scan_device with GTX_READS_UNSORTED on a context whose bucket minimum is one read, into an output
that held a sentinel."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "ibm-cbc-genomic-tools_amd")]

SENTINEL = 0x5A5A5A5A5A5A5A5A


def main(src, dst):
    assert os.environ.get("GTX_BUCKET_MIN_READS") == "1"
    assert os.environ.get("GTX_SCAN_BUCKETS") == "1" or os.environ.get("GTX_SCAN_FUSED") == "0"
    import torch
    import gtx
    z = np.load(src)
    reads, w, qoff, clen, coff, woff = (z[k] for k in ("reads", "weights", "reads_off", "class_len", "class_off", "win_off"))
    dev = torch.device("cuda", 0)
    out = np.zeros((1 + w.shape[0], int(woff[-1])), dtype=np.uint64)
    e = gtx.Engine(0)
    for i in range(len(z["step"])):
        q = np.ascontiguousarray(reads[qoff[i]:qoff[i + 1]])
        n_win = int(woff[i + 1] - woff[i])
        d_reads = torch.from_numpy(q).to(dev)
        for v in range(1 + w.shape[0]):
            d_w = None if v == 0 else torch.from_numpy(np.ascontiguousarray(w[v - 1, qoff[i]:qoff[i + 1]])).to(dev)
            d_out = torch.full((max(n_win, 1),), SENTINEL, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            e.scan_device(d_reads.data_ptr(), len(q), clen[coff[i]:coff[i + 1]], int(z["step"][i]), int(z["size"][i]), d_out.data_ptr(),
                          "c" if z["centre"][i] else "1", None if d_w is None else d_w.data_ptr(), gtx.READS_UNSORTED)
            e.sync()
            out[v, woff[i]:woff[i + 1]] = d_out.cpu().numpy().view(np.uint64)[:n_win]
    e.close()
    np.save(dst, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
