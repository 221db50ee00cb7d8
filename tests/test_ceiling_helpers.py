"""The host side of test_gpu_ceiling.py, without a GPU: the closed-form matrix (tests/ceiling.py) at full parameters and at a
small scale, its shuffled COO, the binned plan's 32-bit guard (parity.binned_fits) and the exact comparison."""
import numpy as np
import pytest

import ceiling as cz
import oracle_binding as ob
import smvp_toolkit_amd as sm
from parity import BIN_BUCKET, BIN_ROW_CAP, binned_fits, binned_regime

torch = pytest.importorskip("torch")

SMALL = dict(rows=4096, nnz=60_000, empty_tail=10, long_min=300)


def test_full_layout_holds_exactly_the_ceiling():
    L = cz.layout()
    assert L["rows"] == 1 << 27 and L["rb"] % 2 == 0 and L["rs"] % 2 == 0
    assert cz.BAND_BASE * L["rb"] + cz.SCAT_BASE * L["rs"] + L["long_len"] == cz.K_MAX == 2147418111
    assert 2048 < L["long_len"] <= 16384 and L["long_len"] < 1 << 20
    assert 0.3 <= (cz.SCAT_BASE * L["rs"] + L["long_len"]) / cz.K_MAX <= 0.4   # the entries far from the diagonal
    total = 0
    for r0 in range(0, L["rows"], 1 << 23):            # the generator's own lengths, summed row chunk by row chunk
        lens = cz.row_lengths(torch, L, r0, min(L["rows"], r0 + (1 << 23)))
        assert int(lens.min()) >= 0
        total += int(lens.sum())
    assert total == cz.K_MAX


@pytest.fixture(scope="module")
def small():
    L = cz.layout(**SMALL)
    rp, ci, v, y = cz.build(torch, L)
    return L, rp.numpy(), ci.numpy(), v.numpy(), y.numpy()


def test_small_layout_structure(small):
    L, rp, ci, v, y = small
    lens = np.diff(rp)
    nnz = SMALL["nnz"]
    assert rp[0] == 0 and rp[-1] == nnz and len(ci) == len(v) == nnz + 1 and ci[nnz] == 0 and v[nnz] == 0
    rb, rs, lr = L["rb"], L["rs"], L["long_row"]
    assert lens[:rb].min() >= 8 and lens[:rb].max() <= 16 and lens[rb:rb + rs].min() >= 1 and lens[rb:rb + rs].max() <= 79
    assert (lens[:rb:2] + lens[1:rb:2] == 2 * cz.BAND_BASE).all() and (lens[rb:lr:2] + lens[rb + 1:lr:2] == 2 * cz.SCAT_BASE).all()
    assert lens[lr] == L["long_len"] >= SMALL["long_min"] and rp[lr + 1] == nnz and (lens[lr + 1:] == 0).all()
    assert len(lens) - lr - 1 >= SMALL["empty_tail"]
    row = np.repeat(np.arange(SMALL["rows"]), lens)
    c = ci[:nnz].astype(np.int64)
    assert (c >= 0).all() and (c < SMALL["rows"]).all()
    band = row < rb
    assert (c[band] == row[band] + 2 + (np.arange(nnz) - rp[row])[band]).all()          # r + 2 ... r + len + 1: none within 1
    inner = np.diff(c) > 0
    assert inner[row[1:] == row[:-1]].all()                                              # ascending and distinct in every row
    assert np.abs(c[~band] - row[~band]).max() > SMALL["rows"] // 2                      # scattered over the columns
    vv = v[:nnz]
    assert (vv == np.round(vv)).all() and (np.abs(vv) >= 1).all() and (np.abs(vv) <= 8).all()
    x = cz.x_int(torch, SMALL["rows"]).numpy()
    assert (np.abs(x) >= 1).all() and (np.abs(x) <= 8).all() and (x > 0).any() and (x < 0).any()


def test_small_reference_is_the_serial_loop(small):
    """The int64 reference equals the C oracle's serial loop (all sums exact) -- and one changed bit in the last row's
    product is flagged by the exact comparison the GPU tests make."""
    L, rp, ci, v, y = small
    x = cz.x_int(torch, SMALL["rows"]).numpy().astype(np.float64)
    ref = ob.csr_spmv(rp, ci[:SMALL["nnz"]], v[:SMALL["nnz"]], x)
    assert np.array_equal(y, ref)
    bad = ref.copy()
    lr = L["long_row"]
    bad[lr] = (bad[lr:lr + 1].view(np.int64) ^ 1).view(np.float64)[0]
    yt, bt = torch.from_numpy(y), torch.from_numpy(bad)
    assert not torch.equal(bt, yt) and int(torch.nonzero(bt != yt).flatten()[0]) == lr


def test_small_coo_is_a_shuffle_of_the_csr(small):
    L, rp, ci, v, y = small
    nnz = SMALL["nnz"]
    a, b = cz.coo_permutation(nnz)
    assert np.unique((np.arange(nnz, dtype=np.int64) * a + b) % nnz).size == nnz
    buf = cz.build_coo(torch, torch.from_numpy(rp), torch.from_numpy(ci), torch.from_numpy(v), nnz, "cpu").numpy()
    coo = buf.view(sm.COO_DTYPE)
    assert len(coo) == nnz and not np.array_equal(coo["row"], np.sort(coo["row"]))
    r2, c2, v2 = sm.csr_from_coo(coo, SMALL["rows"])
    assert np.array_equal(r2, rp) and np.array_equal(c2, ci[:nnz]) and np.array_equal(v2, v[:nnz])


def test_small_far_count_matches_binned_regime(small):
    L, rp, ci, v, y = small
    nnz = SMALL["nnz"]
    for band in (1, 4096, 100):
        nf = cz.binned_far_count(torch, torch.from_numpy(rp), torch.from_numpy(ci[:nnz]), band, BIN_ROW_CAP, chunk=1000)
        assert nf == binned_regime(rp, ci[:nnz], SMALL["rows"], band)["nf"]
    nf1 = cz.binned_far_count(torch, torch.from_numpy(rp), torch.from_numpy(ci[:nnz]), 1, BIN_ROW_CAP)
    assert nf1 >= int(rp[L["rb"]])             # band 1: every banded entry is far


def test_binned_fits_mirrors_the_plan_guard():
    """nf + 256 (ncb + nf / bucket + 2) <= 2147483000 (smvp_binned.hip): the edge, and the two cases of the ceiling test."""
    cols = 1 << 27
    ncb = cols >> 14
    lo, hi = 0, 2 ** 31                        # the least nf the guard refuses, by bisection on its formula
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if mid + 256 * (ncb + mid // BIN_BUCKET + 2) > 2147483000 else (mid, hi)
    edge = hi
    assert 2.07e9 < edge < 2.08e9
    assert binned_fits(edge - 1, cols) and not binned_fits(edge, cols)
    L = cz.layout()
    assert binned_fits(cz.SCAT_BASE * L["rs"], cols)                    # default band: the scattered rows' entries
    assert not binned_fits(cz.K_MAX - L["long_len"], cols)              # band 1: all but the long row
    assert binned_fits(0, 1) and not binned_fits(2147483000, 1)


def test_device_converter_wrappers_refuse_one_entry_more_before_allocating():
    """sm.csr_from_coo_device / tjds_from_coo_device allocate their outputs (26 / 35 GB at the ceiling) only after checking
    the count against the library's limit: one entry more is ERR_UNSUPPORTED at once, with no device touched."""
    assert sm.MAX_ENTRIES == cz.K_MAX
    coo = torch.empty(16, dtype=torch.uint8)
    for f in (sm.csr_from_coo_device, sm.tjds_from_coo_device):
        with pytest.raises(sm.SmvpError) as e:
            f(coo, 1 << 27, 1 << 27, sm.MAX_ENTRIES + 1)
        assert e.value.code == sm.ERR_UNSUPPORTED and "2147418111" in str(e.value)
