"""Phase stamps of one z workgroup (wave 0) at the synthetic config: kernel entry, end of
prologue, then per tile E start, draw start, draw end, XZ operands issued, XZ end (z_kernel.h
Z_STAMP; shader clock cycles).  --wg BY,CHUNK selects the stamped workgroup (species block,
site chunk; default 0,0 -- a chunk past the grid's last means the last), and may be given
several times: one chain per workgroup, since HMSC_Z_STAMP_WG is read at create.  Diagnostic
library only: python -m hmsc_amd.build --stamps; HMSC_AMD_LIB selects another stamps build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HMSC_AMD_LIB", os.path.join(ROOT, "hmsc_amd", "libhmsc_amd_stamps.so"))
import hmsc_amd as H  # noqa: E402
from hmsc_amd.workloads import synthetic_probit  # noqa: E402

wgs = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--wg"] or ["0,0"]
hM = synthetic_probit()
for wg in wgs:
    os.environ["HMSC_Z_STAMP_WG"] = wg
    ch = H.Chain(hM, 1234567, device=0, updater={"GammaEta": False})
    ch.init([10])
    rows = []
    for rep in range(5):  # the last sweep of each short run of captured-graph replays
        ch.run(transient=40, samples=1, thin=1, record=False, iter0=41 * rep)
        ch.sync()
        rows.append(np.array(ch.debug_get("zstamps", 64), dtype=np.float64))
    print("workgroup (species block, site chunk) = (%s), chunks %d" % (wg, int(ch.debug_get("dims", 8)[4])))
    ch.close()
    for st in rows:
        t0 = st[0]
        out = ["prologue %d" % (st[1] - t0)]
        prev = st[1]
        n = 0
        # (the table outlives the chain and the clocks of two compute units need not agree: a slot
        # left by another workgroup's longer chunk is told by its distance from this one's stamps)
        while 2 + 5 * n + 4 < 64 and prev <= st[2 + 5 * n] <= st[2 + 5 * n + 4] < prev + 2.0 ** 20:
            v = st[2 + 5 * n:2 + 5 * n + 5]
            seg = np.diff(np.concatenate([[prev], v]))
            out.append("tile %d: gap %d E %d draw %d loads %d XZ %d" % ((n,) + tuple(int(x) for x in seg)))
            prev = v[4]
            n += 1
        print("z stamps (cycles): total %d | " % (prev - t0) + " | ".join(out))
