#!/usr/bin/env python3
"""A/B in ONE process of the plan option "csr_sweep_alternate": 0 = every product of the tile kernel sweeps its tiles forward
("off"); "on" = the library's default (a handle's plain launches alternate forward / backward where one product's bytes exceed
the Infinity Cache: a product then starts on what the one before it left there) or, with --on 1, alternating whatever the size.
The headline is bimodal from process to process (profiles/r06_headline_variance.txt), so only this separates a few per cent
from that.

Per case: --alternations times (off, on); each setting builds a fresh handle over the SAME adopted device arrays (the option
is read when the plan is built), prewarms, then times --blocks blocks of --steps products between two events; the figure of a
setting is the median block.  A library without the option (the parent build, SMVP_LIB_PATH=...) runs both columns with the
same code: what then differs between the columns, and between the alternations of one column, is the protocol's own spread.

    python3 tools/exp_sweep_direction.py --cases memplus:944:csr,pwt:459:csr,memplus:944:tjds,pwt:459:tjds,memplus:100:csr,memplus:200:csr,memplus:300:csr,memplus:472:csr
"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)

OPTION = "csr_sweep_alternate"   # (--option names another 0 / 1 plan option of the tile kernel, e.g. csr_read_once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="memplus:944:csr", help="comma list of base:copies:format (base memplus | pwt, format csr | tjds)")
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--prewarm", type=int, default=150)
    ap.add_argument("--on", default="default", choices=["default", "1"], help='the "on" column: the library\'s default (alternate where one product exceeds the Infinity Cache) or 1 (alternate whatever the size)')
    ap.add_argument("--option", default=OPTION, help="the plan option the two columns differ in")
    a = ap.parse_args()
    globals()["OPTION"] = a.option
    import torch, smvp_toolkit_amd as sm
    from smvp_toolkit_amd import sharding
    import bench_core as core
    try:
        sm.get_option(OPTION); has_option = True
    except Exception:
        has_option = False
    print("# library %s, option %s: %s; off = 0, on = %s" % (os.path.basename(sm.LIB_PATH), OPTION, "present" if has_option else "ABSENT -- both columns run the same code", a.on), flush=True)
    st = torch.cuda.current_stream()
    for case in a.cases.split(","):
        base, copies, fmt = case.split(":")
        blk = core.build_block(sm, sharding, base + "_tiled", argparse.Namespace(copies=int(copies), scaling="strong"), 0, 1)
        rows, cols, nnz = blk["rows"], blk["cols_total"], blk["nnz"]
        x = torch.ones(cols, dtype=torch.float64, device="cuda"); y = torch.empty(rows, dtype=torch.float64, device="cuda")
        if fmt == "csr":
            dev = tuple(torch.from_numpy(blk[k]).cuda() for k in ("row_ptr", "col_ind", "val"))
            make = lambda: sm.CsrMatrix(rows, cols, *dev)
            product = lambda A: A.spmv(x, y, stream=st)
        else:
            coo = np.zeros(nnz, dtype=sm.COO_DTYPE)
            coo["row"] = np.repeat(np.arange(rows, dtype=np.int32), np.diff(blk["row_ptr"])); coo["col"], coo["val"] = blk["col_ind"], blk["val"]
            d_coo = torch.from_numpy(coo.view(np.uint8)).cuda(); del coo
            tj = sm.tjds_from_coo_device(d_coo, rows, cols, nnz); del d_coo
            make = lambda: sm.TjdsMatrix(tj)
            product = lambda A: A.spmv(y, stream=st)
        del blk
        res = {0: [], 1: []}; name = ""; first_y = None
        for alt in range(a.alternations):
            for on in (0, 1):
                if has_option:
                    sm.set_option(OPTION, (None if a.on == "default" else 1) if on else 0)
                A = make()
                if fmt == "tjds":
                    A.set_x(x, stream=st)
                name, nbytes = A.describe()
                for _ in range(a.prewarm): product(A)
                torch.cuda.synchronize()
                if first_y is None:
                    first_y = y.clone()
                same = bool(torch.equal(y.view(torch.int64), first_y.view(torch.int64)))
                ts = []
                for _ in range(a.blocks):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps): product(A)
                    e1.record(); torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / a.steps)
                med = sorted(ts)[len(ts) // 2]
                res[on].append(med)
                print("  %-8s x%-4s %-4s alt %d %-3s  median %.4f ms  blocks %s  y bit-equal to the first %s" % (
                    base, copies, fmt, alt, "on" if on else "off", med, " ".join("%.4f" % t for t in ts), same), flush=True)
                A.close(); del A
        if has_option:
            sm.set_option(OPTION, None)
        off, on_ = np.array(res[0]), np.array(res[1])
        gains = (off - on_) / off * 100.0
        spread = max((off.max() - off.min()) / off.mean(), (on_.max() - on_.min()) / on_.mean()) * 100.0
        print("%-8s x%-4s %-4s %s | %.0f MB | off %s | on %s | gain %% per alternation %s | mean gain %.2f %% | spread of one setting %.2f %% | %.2f / %.2f TB/s" % (
            base, copies, fmt, name, nbytes * 1e-6, " ".join("%.4f" % t for t in off), " ".join("%.4f" % t for t in on_),
            " ".join("%+.2f" % g for g in gains), float(gains.mean()), spread, nbytes / off.mean() * 1e-9, nbytes / on_.mean() * 1e-9), flush=True)
        del make, product, x, y, first_y
        if fmt == "csr":
            del dev
        else:
            del tj
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
