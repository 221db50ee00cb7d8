#!/usr/bin/env python3
"""The escape-share sweep that fixes AUTO's bound for SMVP_CSR_KERNEL_STREAM_PACKED (kPackedMaxEscapeShare, csrc/smvp_engine.hip),
and the family against STREAM in ONE process on a matrix's own values -- tools/exp_sweep_direction.py's protocol.

Per case base:copies (memplus | pwt) and per share: the case's structure with its values replaced so that the given share of the
entries escapes -- an entry escapes with that probability and then holds a value no other entry has, the others hold one of 32
frequent values; "own" keeps the matrix's values.  --alternations times (STREAM, PACKED): each setting re-plans the one handle over
the SAME adopted device arrays (smvp_csr_set_kernel; both at 2048-entry tiles), prewarms, then times --blocks blocks of --steps
products between two events; a setting's figure is its median block.  y must be bit-equal between the two.  The bound is the
largest share at which PACKED still wins by more than the spread of STREAM's own blocks.

    python3 tools/exp_packed_values.py --cases memplus:944,pwt:459 --shares own,0,0.25,0.5,0.75,1
"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="memplus:944")
    ap.add_argument("--shares", default="own,0,0.25,0.5,0.75,1")
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--prewarm", type=int, default=150)
    a = ap.parse_args()
    import torch, smvp_toolkit_amd as sm
    from smvp_toolkit_amd import sharding
    import bench_core as core
    st = torch.cuda.current_stream()
    print("# library %s" % os.path.basename(sm.LIB_PATH), flush=True)
    for case in a.cases.split(","):
        base, copies = case.split(":")
        blk = core.build_block(sm, sharding, base + "_tiled", argparse.Namespace(copies=int(copies), scaling="strong"), 0, 1)
        rows, cols, nnz = blk["rows"], blk["cols_total"], blk["nnz"]
        x = torch.ones(cols, dtype=torch.float64, device="cuda"); y = torch.empty(rows, dtype=torch.float64, device="cuda")
        d_rp, d_ci = (torch.from_numpy(blk[k]).cuda() for k in ("row_ptr", "col_ind"))
        d_val = torch.from_numpy(blk["val"]).cuda()
        own = blk["val"]; del blk
        A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_val)
        for share in a.shares.split(","):
            if share == "own":
                val = own
            else:
                rng = np.random.default_rng(7)
                val = np.where(rng.random(nnz) < float(share), 1.0 + np.arange(nnz) / float(1 << 32), rng.integers(1, 33, nnz) / 64.0)
            d_val.copy_(torch.from_numpy(val))
            res = {sm.CSR_KERNEL_STREAM: [], sm.CSR_KERNEL_STREAM_PACKED: []}; blocks = {k: [] for k in res}; first_y = None; names = {}
            for alt in range(a.alternations):
                for kernel in res:
                    A.set_kernel(kernel, 2048)
                    names[kernel], nbytes = A.describe()
                    plan = A.plan_info()["plan_bytes"]
                    for _ in range(a.prewarm): A.spmv(x, y, stream=st)
                    torch.cuda.synchronize()
                    if first_y is None:
                        first_y = y.clone()
                    if not torch.equal(y.view(torch.int64), first_y.view(torch.int64)):
                        raise SystemExit("%s share %s: y of %s differs from the first product's" % (case, share, names[kernel]))
                    ts = []
                    for _ in range(a.blocks):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.steps): A.spmv(x, y, stream=st)
                        e1.record(); torch.cuda.synchronize()
                        ts.append(e0.elapsed_time(e1) / a.steps)
                    res[kernel].append(sorted(ts)[len(ts) // 2]); blocks[kernel] += ts
                    if kernel == sm.CSR_KERNEL_STREAM_PACKED:
                        packed_plan = plan
                    else:
                        stream_plan = plan
            s, p = np.array(res[sm.CSR_KERNEL_STREAM]), np.array(res[sm.CSR_KERNEL_STREAM_PACKED])
            sb = np.array(blocks[sm.CSR_KERNEL_STREAM])
            esc_bytes = packed_plan - stream_plan - nnz      # 8 per escape slot (+ table and run starts)
            print("%-8s x%-4s share %-5s | STREAM %s | PACKED %s | gain %% per alternation %s | mean gain %+.2f %% | spread of STREAM's blocks %.2f %% | "
                  "escape slots / nnz %.3f | y bit-equal checked (a difference ends the run)" % (
                      base, copies, share, " ".join("%.4f" % t for t in s), " ".join("%.4f" % t for t in p),
                      " ".join("%+.2f" % g for g in (s - p) / s * 100.0), float(((s - p) / s).mean() * 100.0),
                      (sb.max() - sb.min()) / sb.mean() * 100.0, esc_bytes / 8.0 / nnz), flush=True)
        A.close()
        del A, d_rp, d_ci, d_val, x, y, first_y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
