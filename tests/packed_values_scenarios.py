"""The scenario of tests/test_gpu_packed_values.py::test_allocations_return_to_their_start: `python packed_values_scenarios.py` in a
fresh process whose SMVP_LIB_PATH names lib/libsmvp_amd_counted.so.  Every way the packed family's arrays come and go -- set by
name, picked by AUTO, tried by AUTO and dropped because the escape share is over the bound, refused, replaced by another plan,
re-planned in place -- gives back every device allocation it took; with fresh allocations filled, the products are still STREAM's.
"packed values ok" is the last line of a run that passed.
"""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs
import packed_values as pv

sm = rs.sm
PACKED, STREAM = sm.CSR_KERNEL_STREAM_PACKED, sm.CSR_KERNEL_STREAM


def main():
    import torch

    if not hasattr(sm.lib(), "smvp_test_resources"):
        print("FAIL: %s is not the counted build (set SMVP_LIB_PATH to lib/libsmvp_amd_counted.so)" % sm.LIB_PATH)
        return 1
    rows, cols, rp, ci = pv.base()
    under, over = pv.values("third", rp, ci), pv.values("distinct", rp, ci)
    x = torch.from_numpy(np.random.default_rng(1).random(cols)).cuda()
    y = torch.empty(rows, dtype=torch.float64, device="cuda")
    want = torch.empty_like(y)

    def multiply(A, out):
        A.spmv(x, out, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()

    try:
        with rs.balanced("set by name, re-planned in place, replaced by STREAM and by VECTOR, set again"):
            A = sm.CsrMatrix(rows, cols, rp, ci, under)
            A.set_kernel(STREAM, 2048)
            multiply(A, want)
            held_stream = rs.at(rs.snap(), rs.DEVICE, rs.LIVE)
            for kernel, param in ((PACKED, 0), (PACKED, 2048), (STREAM, 2048), (PACKED, 0), (sm.CSR_KERNEL_VECTOR, 0), (PACKED, 0)):
                A.set_kernel(kernel, param)
                if kernel == PACKED:
                    rs.expect(rs.at(rs.snap(), rs.DEVICE, rs.LIVE) == held_stream + 4, "the packed plan holds four arrays more than STREAM's")
                    multiply(A, y)
                    rs.expect(torch.equal(y.view(torch.int64), want.view(torch.int64)), "the packed product is not STREAM's")
            A.close()
        with rs.balanced("picked by AUTO; tried by AUTO and dropped; never tried"):
            for val, packed, kernel in ((under, 1, PACKED), (over, 1, STREAM), (under, 0, STREAM), (under, None, STREAM)):
                with sm.option("csr_packed", packed):
                    A = sm.CsrMatrix(rows, cols, rp, ci, val)
                rs.expect(A.get_kernel()[0] == kernel, "AUTO under csr_packed %r picked %r" % (packed, A.get_kernel()))
                multiply(A, y)
                A.close()
        with rs.balanced("refused: no 16-bit offsets"):
            with sm.option("csr_col16", 0):
                A = sm.CsrMatrix(rows, cols, rp, ci, under)
                rs.expect(rs.status("smvp_csr_set_kernel", A._h, PACKED, 0) == sm.ERR_UNSUPPORTED, "set_kernel without offsets is not refused")
            multiply(A, y)
            A.close()
        # fresh allocations filled with a pattern (tests/resource_count.cpp): nothing the packed plan leaves unwritten reaches y
        lib = sm.lib()
        lib.smvp_test_fill_allocations.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
        for mode in (1, 2):
            rs.expect(lib.smvp_test_fill_allocations(mode, 0, -1) == 0, "smvp_test_fill_allocations(%d) was refused" % mode)
            with rs.balanced("fill mode %d" % mode):
                for val in (under, over):
                    A = sm.CsrMatrix(rows, cols, rp, ci, val)
                    A.set_kernel(STREAM, 2048)
                    multiply(A, want)
                    A.set_kernel(PACKED, 0)
                    multiply(A, y)
                    rs.expect(torch.equal(y.view(torch.int64), want.view(torch.int64)), "fill mode %d: the packed product is not STREAM's" % mode)
                    A.close()
        lib.smvp_test_fill_allocations(0, 0, 0)
    except rs.Failed as e:
        print("FAIL: %s" % e)
        return 1
    for what in rs.DONE:
        print("ok  %s" % what)
    print("packed values ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
