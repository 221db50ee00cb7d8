// host_san_driver.cpp -- exercises the host side of libsmvp_amd under sanitizers (make -C smvp-toolkit_amd host-san).
//
// Not part of the product: a test driver linked against the ten host translation units only (reader, converters,
// report writer, cache, CISR export, synthetic generators, the triangular solves' analysis, the ILU(0) check and host loop, LSQR's
// argument check, error text -- no HIP), built with
// g++ -fsanitize=address,undefined and, for the parallel Matrix Market tokeniser, -fsanitize=thread (SURVEY 5,
// "race detection / sanitizers": the reference has none, CMakeLists.txt:33-34 even comments -Wall out).
// tests/test_host_sanitizers.py runs it over the reference's sample files, malformed inputs, crafted cache files.
//
//   host_san_driver file <path.mtx> <tmpdir>   everything the host library does with one input file
//   host_san_driver cache <file.smvpbin> <path.mtx>   a cache file somebody else wrote (crafted ones in the tests)
//   host_san_driver synth <tmpdir>              the generators, the partition, the report writer's edge cases
// Exit status 0 unless a call that must succeed fails (an input the library REJECTS is a pass: what is looked for is what the
// sanitizer reports, which ends the process by itself).
#include "smvp_amd.h"
#include "smvp_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

static int g_bad = 0;
#define MUST(expr)                                                                     \
    do {                                                                               \
        const int rc_ = (expr);                                                        \
        if (rc_ != SMVP_OK) {                                                          \
            fprintf(stderr, "FAILED %s -> %d (%s)\n", #expr, rc_, smvp_last_error());  \
            ++g_bad;                                                                   \
        }                                                                              \
    } while (0)

static int run_file(const char *path, const std::string &tmp)
{
    smvp_mm_typecode tc;
    int rows = 0, cols = 0, nnz = 0;
    int rc = smvp_mm_read_header_path(path, &tc, &rows, &cols, &nnz);
    printf("header: rc %d rows %d cols %d nnz %d (%s)\n", rc, rows, cols, nnz, rc ? smvp_last_error() : "ok");
    if (rc != SMVP_OK)
        return 0;  // rejected: fine
    if (nnz < 0 || rows < 0 || cols < 0 || nnz > 50 * 1000 * 1000)
        return 0;
    std::vector<smvp_coo_t> coo((size_t)nnz + 1);
    rc = smvp_mm_read_coo_path(path, coo.data(), nnz, &tc, &rows, &cols, &nnz);
    printf("entries: rc %d (%s)\n", rc, rc ? smvp_last_error() : "ok");
    if (rc != SMVP_OK)
        return 0;
    // the reader through FILE* as well (what the command line does)
    if (FILE *f = fopen(path, "r")) {
        smvp_mm_typecode tc2;
        int r2, c2, n2;
        if (smvp_mm_read_banner(f, &tc2) == SMVP_OK && smvp_mm_read_mtx_crd_size(f, &r2, &c2, &n2) == SMVP_OK && n2 == nnz) {
            std::vector<smvp_coo_t> again((size_t)nnz + 1);
            MUST(smvp_mm_read_coo_entries(f, tc2, nnz, again.data()));
            if (memcmp(again.data(), coo.data(), sizeof(smvp_coo_t) * (size_t)nnz) != 0) {
                fprintf(stderr, "FAILED: the two readers disagree\n");
                ++g_bad;
            }
        }
        fclose(f);
    }
    bool inside = true;
    for (int i = 0; i < nnz; ++i)
        inside = inside && coo[(size_t)i].row >= 0 && coo[(size_t)i].row < rows && coo[(size_t)i].col >= 0 && coo[(size_t)i].col < cols;
    printf("entries inside the matrix: %d\n", (int)inside);
    // ---- COO -> CSR, CSR -> COO
    std::vector<int> row_ptr((size_t)rows + 1), col_ind((size_t)nnz + 1);
    std::vector<double> val((size_t)nnz + 1);
    rc = smvp_csr_from_coo(coo.data(), rows, nnz, row_ptr.data(), col_ind.data(), val.data());
    printf("csr_from_coo: rc %d\n", rc);
    if (rc == SMVP_OK) {
        std::vector<smvp_coo_t> back((size_t)nnz + 1);
        MUST(smvp_coo_from_csr(rows, row_ptr.data(), col_ind.data(), val.data(), back.data()));
        std::vector<int> bounds(9);
        MUST(smvp_partition_rows(row_ptr.data(), rows, 8, bounds.data()));
        // ---- the binary cache: write, read the header and the arrays back, then a cache made from OTHER bytes
        const std::string cache = tmp + "/m.smvpbin";
        MUST(smvp_cache_write_csr(cache.c_str(), path, tc, 0, rows, cols, nnz, row_ptr.data(), col_ind.data(), val.data()));
        smvp_mm_typecode tc3;
        int fl = 0, r3 = 0, c3 = 0, n3 = 0;
        MUST(smvp_cache_read_header(cache.c_str(), path, &tc3, &fl, &r3, &c3, &n3));
        if (r3 == rows && n3 == nnz) {
            std::vector<int> rp2((size_t)rows + 1), ci2((size_t)nnz + 1);
            std::vector<double> v2((size_t)nnz + 1);
            MUST(smvp_cache_read_csr(cache.c_str(), rows, nnz, rp2.data(), ci2.data(), v2.data()));
        }
        // truncated and bit-flipped caches must be refused, not read past
        if (FILE *f = fopen(cache.c_str(), "rb")) {
            std::vector<unsigned char> bytes;
            unsigned char b[4096];
            size_t got;
            while ((got = fread(b, 1, sizeof b, f)) > 0)
                bytes.insert(bytes.end(), b, b + got);
            fclose(f);
            for (int variant = 0; variant < 4 && bytes.size() > 80; ++variant) {
                std::vector<unsigned char> bad = bytes;
                if (variant == 0)
                    bad.resize(bad.size() / 2);
                else if (variant == 1)
                    bad.resize(40);
                else if (variant == 2)
                    bad[bad.size() - 9] ^= 0x40;  // an array byte: the checksum must catch it
                else
                    bad[70 % bad.size()] ^= 0xff;  // (past the 64-byte header: row_ptr)
                const std::string p2 = tmp + "/bad.smvpbin";
                if (FILE *g = fopen(p2.c_str(), "wb")) {
                    fwrite(bad.data(), 1, bad.size(), g);
                    fclose(g);
                    int rr = 0, cc = 0, nn = 0, ff = 0;
                    smvp_mm_typecode t4;
                    int hrc = smvp_cache_read_header(p2.c_str(), path, &t4, &ff, &rr, &cc, &nn);
                    if (hrc == SMVP_OK && rr == rows && nn == nnz) {
                        std::vector<int> rp2((size_t)rows + 1), ci2((size_t)nnz + 1);
                        std::vector<double> v2((size_t)nnz + 1);
                        hrc = smvp_cache_read_csr(p2.c_str(), rows, nnz, rp2.data(), ci2.data(), v2.data());
                    }
                    printf("crafted cache %d: rc %d\n", variant, hrc);
                    if (hrc == SMVP_OK) {
                        fprintf(stderr, "FAILED: a damaged cache file was accepted\n");
                        ++g_bad;
                    }
                }
            }
        }
    }
    // ---- COO -> TJDS
    if (inside) {
        std::vector<int> perm((size_t)cols + 1), sp((size_t)(rows > nnz ? rows : nnz) + 2), ri((size_t)nnz + 1);
        std::vector<double> tv((size_t)nnz + 1);
        int nd = 0, refn = 0, single = 0;
        rc = smvp_tjds_from_coo(coo.data(), rows, cols, nnz, perm.data(), sp.data(), (int)sp.size(), ri.data(), tv.data(), &nd, &refn, &single);
        printf("tjds_from_coo: rc %d diagonals %d ref %d single %d\n", rc, nd, refn, single);
        // too small a start_pos: refused, not overrun
        if (nd > 1) {
            std::vector<int> tiny((size_t)nd);  // needs nd + 1
            int rc2 = smvp_tjds_from_coo(coo.data(), rows, cols, nnz, perm.data(), tiny.data(), nd, ri.data(), tv.data(), &nd, nullptr, nullptr);
            printf("tjds_from_coo with a short start_pos: rc %d\n", rc2);
        }
    }
    // ---- symmetric expansion
    int count = 0;
    rc = smvp_mm_expanded_count(tc, coo.data(), nnz, &count);
    if (rc == SMVP_OK && count >= nnz && count < 120 * 1000 * 1000) {
        std::vector<smvp_coo_t> full((size_t)count + 1);
        int n_out = 0;
        rc = smvp_mm_expand_symmetric(tc, coo.data(), nnz, rows, cols, full.data(), count, &n_out);
        printf("expand: rc %d %d -> %d\n", rc, nnz, n_out);
        if (count > nnz) {  // too small a buffer: refused
            int rc2 = smvp_mm_expand_symmetric(tc, coo.data(), nnz, rows, cols, full.data(), count - 1, &n_out);
            printf("expand into a short buffer: rc %d\n", rc2);
        }
    }
    // ---- CISR export with 1 and 16 slots (1 is where the reference "overruns", main-cli.c:596-600), small matrices only
    if (inside && rows > 0 && nnz <= 400000) {
        for (int slots : {1, 16, 3}) {
            FILE *out = fopen((tmp + "/m.coe").c_str(), "w");
            if (!out)
                continue;
            rc = smvp_cisr_coegen(coo.data(), rows, nnz, slots, out);
            fclose(out);
            printf("cisr %d slots: rc %d\n", slots, rc);
        }
    }
    // ---- report writer
    if (rows > 0) {
        std::vector<double> y((size_t)rows, 1.5), each(7, 0.25);
        smvp_time_stats_t st;
        MUST(smvp_time_stats(each.data(), 7, &st));
        char outp[4096];
        MUST(smvp_generate_report_text(path, tmp.c_str(), "CSR", nnz, rows, 7, y.data(), &st, 1615284655ul, outp, sizeof outp));
        MUST(smvp_generate_report_text(path, (tmp + "/").c_str(), "TJDS", nnz, rows, 7, y.data(), &st, 0ul, outp, 8));  // short out_path
    }
    return 0;
}

static int run_synth(const std::string &tmp)
{
    for (int kind : {SMVP_SYNTH_MEMPLUS_SHAPED, SMVP_SYNTH_UNIFORM}) {
        const int64_t total = 20000, r0 = 3000, r1 = 9000;
        std::vector<int> lens((size_t)(r1 - r0)), rp((size_t)(r1 - r0) + 1, 0);
        MUST(smvp_synth_row_lengths(kind, 12345, total, total, 32, r0, r1, lens.data()));
        for (size_t i = 0; i < lens.size(); ++i)
            rp[i + 1] = rp[i] + lens[i];
        std::vector<int> ci((size_t)rp.back() + 1);
        std::vector<double> v((size_t)rp.back() + 1);
        for (int threads : {1, 4})
            MUST(smvp_synth_fill(kind, 12345, total, total, 32, r0, r1, rp.data(), ci.data(), v.data(), threads));
        for (size_t i = 0; i + 1 < rp.size(); ++i)
            for (int j = rp[i]; j < rp[i + 1]; ++j)
                if (ci[(size_t)j] < 0 || ci[(size_t)j] >= total || (j > rp[i] && ci[(size_t)j] <= ci[(size_t)j - 1])) {
                    fprintf(stderr, "FAILED: synthetic row %zu is not sorted / inside\n", i);
                    return ++g_bad;
                }
        std::vector<int> bounds(6);
        MUST(smvp_partition_rows(rp.data(), (int)(r1 - r0), 5, bounds.data()));
    }
    std::vector<double> x(1001);
    MUST(smvp_vector_random(x.data(), 1001, 67890));
    // empty and degenerate inputs
    smvp_time_stats_t st;
    double one = 3.0;
    MUST(smvp_time_stats(&one, 1, &st));
    (void)smvp_time_stats(nullptr, 0, &st);
    std::vector<int> rp1(1, 0), b(3);
    MUST(smvp_partition_rows(rp1.data(), 0, 2, b.data()));
    int rc = smvp_csr_from_coo(nullptr, 0, 0, rp1.data(), nullptr, nullptr);
    printf("empty csr_from_coo: rc %d\n", rc);
    char outp[64];
    rc = smvp_generate_report_text("x.mtx", (tmp + "/no/such/dir").c_str(), "CSR", 0, 0, 1, nullptr, &st, 1ul, outp, sizeof outp);
    printf("report into a missing directory: rc %d\n", rc);
    // ---- K15's host analysis (smvp_trsv_plan.cpp): empty, one row, a chain, unsorted columns with repeats, arrays it must refuse
    int levels = -1;
    MUST(smvp_csr_trsv_levels(0, rp1.data(), nullptr, SMVP_TRSV_LOWER, nullptr, &levels));
    MUST(smvp_csr_trsv_levels(0, nullptr, nullptr, SMVP_TRSV_UPPER, nullptr, &levels));
    std::vector<int> lone{0, 2}, lone_c{0, 0}, lv(8, -1);
    MUST(smvp_csr_trsv_levels(1, lone.data(), lone_c.data(), SMVP_TRSV_UPPER, lv.data(), &levels));
    if (levels != 1 || lv[0] != 0)
        ++g_bad, fprintf(stderr, "FAILED: one row has %d levels, level %d\n", levels, lv[0]);
    const int n = 5000;
    std::vector<int> chain_rp((size_t)n + 1), chain_c, chain_lv((size_t)n);
    for (int i = 0; i < n; ++i) {  // (i, i) and (i, i - 1): n levels for LOWER, one for UPPER
        chain_rp[(size_t)i] = (int)chain_c.size();
        chain_c.push_back(i);
        if (i)
            chain_c.push_back(i - 1);
    }
    chain_rp[(size_t)n] = (int)chain_c.size();
    MUST(smvp_csr_trsv_levels(n, chain_rp.data(), chain_c.data(), SMVP_TRSV_LOWER, chain_lv.data(), &levels));
    if (levels != n || chain_lv[(size_t)n - 1] != n - 1)
        ++g_bad, fprintf(stderr, "FAILED: the chain has %d levels\n", levels);
    MUST(smvp_csr_trsv_levels(n, chain_rp.data(), chain_c.data(), SMVP_TRSV_UPPER, chain_lv.data(), &levels));
    if (levels != 1)
        ++g_bad, fprintf(stderr, "FAILED: the chain's upper triangle has %d levels\n", levels);
    std::vector<int> mix_rp{0, 2, 5, 9, 9}, mix_c{3, 0, 1, 0, 0, 2, 1, 1, 0};  // unsorted, repeated, an empty last row
    for (int uplo : {SMVP_TRSV_LOWER, SMVP_TRSV_UPPER})
        MUST(smvp_csr_trsv_levels(4, mix_rp.data(), mix_c.data(), uplo, lv.data(), &levels));
    if (levels != 2 || lv[0] != 1 || lv[3] != 0)
        ++g_bad, fprintf(stderr, "FAILED: the mixed case's upper triangle: %d levels, row 0 at %d\n", levels, lv[0]);
    // K21's storage ranges on the same arrays: row 0 (columns 3 0) has nothing in its lower triangle under a unit diagonal and
    // its diagonal at position 1 with the stored one, row 2 (columns 2 1 1 0) its diagonal first, the empty row an empty range
    for (int uplo : {SMVP_TRSV_LOWER, SMVP_TRSV_UPPER})
        for (int diag : {SMVP_TRSV_DIAG_STORED, SMVP_TRSV_DIAG_UNIT}) {
            std::vector<int> begin, end;
            long long inside = 0;
            int longest = 0;
            smvp::trsv_ranges(4, mix_rp.data(), mix_c.data(), uplo, diag, &begin, &end, &inside, &longest);
            const bool lower = uplo == SMVP_TRSV_LOWER, stored = diag == SMVP_TRSV_DIAG_STORED;
            if (begin[3] != 9 || end[3] != 9 || (lower && (begin[0] != (stored ? 1 : 0) || end[0] != (stored ? 2 : 0) || begin[2] != (stored ? 5 : 6) || end[2] != 9)))
                ++g_bad, fprintf(stderr, "FAILED: the mixed case's ranges, uplo %d, diag %d\n", uplo, diag);
            long long sum = 0;
            for (int i = 0; i < 4; ++i)
                sum += end[(size_t)i] - begin[(size_t)i];
            if (sum != inside || longest > 4)
                ++g_bad, fprintf(stderr, "FAILED: the mixed case's range total, uplo %d, diag %d\n", uplo, diag);
        }
    mix_c[4] = 4;  // a column past the last row, a decreasing row_ptr, a bad uplo, null arrays: refused before anything is read or written
    rc = smvp_csr_trsv_levels(4, mix_rp.data(), mix_c.data(), SMVP_TRSV_UPPER, lv.data(), &levels);
    mix_c[4] = 0, mix_rp[2] = 1;
    rc += smvp_csr_trsv_levels(4, mix_rp.data(), mix_c.data(), SMVP_TRSV_LOWER, lv.data(), &levels);
    rc += smvp_csr_trsv_levels(4, mix_rp.data(), mix_c.data(), 2, lv.data(), &levels);
    rc += smvp_csr_trsv_levels(4, nullptr, mix_c.data(), SMVP_TRSV_LOWER, lv.data(), &levels);
    rc += smvp_csr_trsv_levels(4, mix_rp.data(), mix_c.data(), SMVP_TRSV_LOWER, nullptr, nullptr);
    printf("five refused trsv analyses: rc sum %d\n", rc);
    if (rc != 5 * SMVP_ERR_INVALID)
        ++g_bad;
    // ---- K17's host side (smvp_ilu0_plan.cpp): the check and the serial factorisation on a small matrix, empty input, refusals
    {
        const std::vector<int> rp3{0, 2, 5, 7}, ci3{0, 1, 0, 1, 2, 1, 2};  // [[4, 2, 0], [2, 5, 2], [0, 2, 2]]
        const std::vector<double> v3{4, 2, 2, 5, 2, 2, 2}, want{4, 2, 0.5, 4, 2, 0.5, 1};
        std::vector<int> dp(3, -1);
        std::vector<double> f3(7, -1.0);
        int bad = 7;
        MUST(smvp_csr_ilu0_check(3, rp3.data(), ci3.data(), dp.data(), &bad));
        MUST(smvp_csr_ilu0_check(3, rp3.data(), ci3.data(), nullptr, nullptr));
        MUST(smvp_csr_ilu0_host(3, rp3.data(), ci3.data(), v3.data(), f3.data()));
        if (bad != -1 || dp != std::vector<int>{0, 3, 6} || f3 != want)
            ++g_bad, fprintf(stderr, "FAILED: the 3 x 3 ILU(0): bad_row %d, diag_pos %d %d %d\n", bad, dp[0], dp[1], dp[2]);
        std::vector<double> in_place(v3);
        MUST(smvp_csr_ilu0_host(3, rp3.data(), ci3.data(), in_place.data(), in_place.data()));
        if (in_place != want)
            ++g_bad, fprintf(stderr, "FAILED: the 3 x 3 ILU(0) in place\n");
        MUST(smvp_csr_ilu0_check(0, rp1.data(), nullptr, nullptr, &bad));
        MUST(smvp_csr_ilu0_host(0, nullptr, nullptr, nullptr, nullptr));
        // the bidiagonal chain above stores (i, i) before (i, i - 1): not ascending, refused at row 1; then the same rows sorted
        int rc17 = smvp_csr_ilu0_check(n, chain_rp.data(), chain_c.data(), chain_lv.data(), &bad);
        if (rc17 != SMVP_ERR_UNSUPPORTED || bad != 1)
            ++g_bad, fprintf(stderr, "FAILED: the unsorted chain: rc %d, bad_row %d\n", rc17, bad);
        for (int i = 1; i < n; ++i)
            std::swap(chain_c[(size_t)chain_rp[(size_t)i]], chain_c[(size_t)chain_rp[(size_t)i] + 1]);
        std::vector<double> cv(chain_c.size(), 0.25), cf(chain_c.size());
        for (int i = 0; i < n; ++i)
            cv[(size_t)chain_rp[(size_t)i + 1] - 1] = 2.0;  // the diagonal stands last in every row
        MUST(smvp_csr_ilu0_host(n, chain_rp.data(), chain_c.data(), cv.data(), cf.data()));
        if (cf[0] != 2.0 || cf[1] != 0.125 || cf[2] != 2.0)  // (row 0 stores no column 1: nothing is subtracted from u_11)
            ++g_bad, fprintf(stderr, "FAILED: the sorted chain's factor begins %g %g %g\n", cf[0], cf[1], cf[2]);
        std::vector<int> no_diag{0, 1, 0, 1, 2, 0, 1}, past{0, 1, 0, 1, 3, 1, 2}, falling{0, 5, 2, 7};
        rc17 = smvp_csr_ilu0_check(3, rp3.data(), no_diag.data(), dp.data(), &bad) == SMVP_ERR_UNSUPPORTED && bad == 2;
        rc17 += smvp_csr_ilu0_host(3, rp3.data(), past.data(), v3.data(), f3.data()) == SMVP_ERR_INVALID;
        rc17 += smvp_csr_ilu0_check(3, falling.data(), ci3.data(), dp.data(), &bad) == SMVP_ERR_INVALID && bad == 1;
        rc17 += smvp_csr_ilu0_check(-1, nullptr, nullptr, nullptr, nullptr) == SMVP_ERR_INVALID;
        rc17 += smvp_csr_ilu0_host(3, rp3.data(), ci3.data(), nullptr, f3.data()) == SMVP_ERR_INVALID;
        printf("five refused ILU(0) calls: %d as expected\n", rc17);
        if (rc17 != 5 || dp != std::vector<int>{0, 3, 6} || f3 != want)
            ++g_bad, fprintf(stderr, "FAILED: a refused ILU(0) call wrote its outputs\n");
    }
    // ---- K22's host side (smvp_lsqr_args.cpp): the defaults, and what smvp_csr_lsqr / smvp_tjds_lsqr refuse before any HIP call, through
    // the check both entry points make first (a block of zeros stands in for a handle: it is not looked at)
    {
        smvp_lsqr_opts_t ok;
        smvp_lsqr_opts_default(&ok);
        smvp_lsqr_opts_default(nullptr);
        if (ok.struct_size != sizeof ok || ok.max_steps != 100 || ok.check_every != 10 || ok.tol != 1e-10 || ok.atol != 1e-10)
            ++g_bad, fprintf(stderr, "FAILED: the LSQR defaults\n");
        const std::vector<char> fake(64, 0);
        const void *h = fake.data(), *ht = fake.data() + 32;
        smvp_lsqr_result_t res;
        const double b = 1.0;
        for (const char *fn : {"smvp_csr_lsqr", "smvp_tjds_lsqr"}) {
            const bool csr = fn[5] == 'c';
            MUST(smvp::lsqr_check_args(fn, h, csr ? ht : nullptr, csr, &ok, &res, &b));
            int refused = smvp::lsqr_check_args(fn, nullptr, ht, csr, &ok, &res, &b) == SMVP_ERR_INVALID;
            refused += smvp::lsqr_check_args(fn, h, nullptr, true, &ok, &res, &b) == SMVP_ERR_INVALID;
            refused += smvp::lsqr_check_args(fn, h, ht, csr, nullptr, &res, &b) == SMVP_ERR_INVALID;
            refused += smvp::lsqr_check_args(fn, h, ht, csr, &ok, nullptr, &b) == SMVP_ERR_INVALID;
            refused += smvp::lsqr_check_args(fn, h, ht, csr, &ok, &res, nullptr) == SMVP_ERR_INVALID;
            const double nan = std::strtod("nan", nullptr), inf = std::strtod("inf", nullptr);
            for (int which = 0; which < 10; ++which) {
                smvp_lsqr_opts_t o = ok;
                switch (which) {
                case 0: o.struct_size = 0; break;
                case 1: o.struct_size = sizeof o - 8; break;
                case 2: o.max_steps = 0; break;
                case 3: o.check_every = 0; break;
                case 4: o.tol = -1e-300; break;
                case 5: o.tol = nan; break;
                case 6: o.tol = inf; break;
                case 7: o.atol = -1e-300; break;
                case 8: o.atol = nan; break;
                default: o.atol = inf; break;
                }
                refused += smvp::lsqr_check_args(fn, h, ht, csr, &o, &res, &b) == SMVP_ERR_INVALID;
            }
            printf("%s: %d of 15 bad argument lists refused\n", fn, refused);
            if (refused != 15)
                ++g_bad;
        }
    }
    // ---- K23's host side (smvp_reorder_host.cpp): the defaults, the checks of the two structs, and the colouring of the chain (two
    // colours on a path whatever the seed), of the unsorted pattern with repeats and an empty row, alone and with itself as the
    // second pattern, of a matrix without rows, and of arrays it must refuse
    {
        smvp_color_opts_t o;
        smvp_color_opts_default(&o);
        smvp_color_opts_default(nullptr);
        smvp_color_info_t ci23{};
        ci23.struct_size = sizeof ci23;
        int bad23 = o.struct_size != sizeof o || o.seed != 0 || o.max_rounds != 4096 || smvp::color_check_opts("smvp_csr_color", &o, &ci23) != SMVP_OK ||
                    smvp::color_check_opts("smvp_csr_color", nullptr, nullptr) != SMVP_OK;
        o.max_rounds = 0;
        bad23 += smvp::color_check_opts("smvp_csr_color", &o, nullptr) != SMVP_ERR_INVALID;
        o.max_rounds = 1, o.struct_size = 8;
        bad23 += smvp::color_check_opts("smvp_csr_color", &o, nullptr) != SMVP_ERR_INVALID;
        ci23.struct_size = 4;
        bad23 += smvp::color_check_opts("smvp_csr_color", nullptr, &ci23) != SMVP_ERR_INVALID;
        int colors = -1, depth = -1;
        mix_rp[2] = 5;  // (as it was before the refused analyses above)
        for (unsigned seed : {0u, 1u, 0xffffffffu}) {
            MUST(smvp_csr_color_host(n, chain_rp.data(), chain_c.data(), nullptr, nullptr, seed, chain_lv.data(), &colors, &depth));
            // (i, i - 1) stored in one direction only: without the second pattern a vertex sees its predecessor alone
            bad23 += colors != 2 || depth < 2;
            MUST(smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), nullptr, nullptr, seed, lv.data(), &colors, &depth));
            bad23 += colors < 1 || colors > 3 || lv[3] != 0;
            MUST(smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), mix_rp.data(), mix_c.data(), seed, lv.data(), &colors, &depth));
            bad23 += colors < 1 || colors > 3;
        }
        MUST(smvp_csr_color_host(0, nullptr, nullptr, nullptr, nullptr, 7, nullptr, &colors, &depth));
        bad23 += colors != 0 || depth != 0;
        int refused = smvp_csr_color_host(-1, mix_rp.data(), mix_c.data(), nullptr, nullptr, 0, lv.data(), &colors, &depth) == SMVP_ERR_INVALID;
        refused += smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), mix_rp.data(), nullptr, 0, lv.data(), &colors, &depth) == SMVP_ERR_INVALID;
        refused += smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), nullptr, nullptr, 0, nullptr, &colors, &depth) == SMVP_ERR_INVALID;
        refused += smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), nullptr, nullptr, 0, lv.data(), nullptr, &depth) == SMVP_ERR_INVALID;
        mix_c[4] = 4;
        refused += smvp_csr_color_host(4, mix_rp.data(), mix_c.data(), nullptr, nullptr, 0, lv.data(), &colors, &depth) == SMVP_ERR_INVALID;
        mix_c[4] = 0;
        printf("K23's host side: %d unexpected results, %d of 5 bad argument lists refused\n", bad23, refused);
        if (bad23 || refused != 5)
            ++g_bad;
    }
    printf("version %s\n", smvp_version_string());
    return 0;
}

// a cache file as somebody else wrote it (tests craft ones whose checksum matches but whose arrays do not hold together)
static int run_cache(const char *cache, const char *mtx)
{
    smvp_mm_typecode tc;
    int flags = 0, rows = 0, cols = 0, nnz = 0;
    int rc = smvp_cache_read_header(cache, mtx, &tc, &flags, &rows, &cols, &nnz);
    printf("cache header: rc %d rows %d cols %d nnz %d\n", rc, rows, cols, nnz);
    if (rc != SMVP_OK || rows < 0 || nnz < 0 || nnz > 50 * 1000 * 1000)
        return 0;
    std::vector<int> rp((size_t)rows + 1), ci((size_t)nnz + 1);
    std::vector<double> v((size_t)nnz + 1);
    rc = smvp_cache_read_csr(cache, rows, nnz, rp.data(), ci.data(), v.data());
    printf("cache arrays: rc %d (%s)\n", rc, rc ? smvp_last_error() : "ok");
    if (rc == SMVP_OK) {
        std::vector<smvp_coo_t> coo((size_t)nnz + 1);
        MUST(smvp_coo_from_csr(rows, rp.data(), ci.data(), v.data(), coo.data()));
    }
    return 0;
}

int main(int argc, char **argv)
{
    // (this test driver, not the library, reads the environment: the reader's thread count for the run)
    if (const char *e = getenv("SMVP_MM_THREADS"))
        (void)smvp_set_option("mm_threads", atoi(e));
    if (argc >= 4 && !strcmp(argv[1], "file"))
        run_file(argv[2], argv[3]);
    else if (argc >= 4 && !strcmp(argv[1], "cache"))
        run_cache(argv[2], argv[3]);
    else if (argc >= 3 && !strcmp(argv[1], "synth"))
        run_synth(argv[2]);
    else {
        fprintf(stderr, "usage: %s file <path.mtx> <tmpdir> | cache <file.smvpbin> <path.mtx> | synth <tmpdir>\n", argv[0]);
        return 2;
    }
    if (g_bad)
        fprintf(stderr, "%d check(s) failed\n", g_bad);
    return g_bad ? 1 : 0;
}
