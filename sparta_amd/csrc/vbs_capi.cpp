// vbs_capi.cpp -- the device image of a VBS matrix (sparta_vbs) and the C-ABI entry points that create, multiply and destroy
// it: sparta_vbs_create* / sparta_vbs_spmm* / sparta_pack_blocks (include/sparta_amd.h).  Host code only: kernels live in the
// k_*.hip translation units and are reached through the launch functions of vbs_device.hpp.
//
// What it replaces in the reference: the CPU triple loop VBR::multiply (src/general/vbr.cpp:323-372)
// and the "one library GEMM per nonzero block" GPU back-ends (src/cuda/cuda_utilities.cpp:39-887,
// src/cuda/cutlass_bellpack_lib.cu:380-1019).  Not a translation of either: there is ONE fused kernel
// family, no vendor BLAS/SPARSE call, no per-block launch.
//
// Elsewhere: the entries that make no HIP call (vbs_host_check.cpp), the epilogue of a linear layer (vbs_epilogue.cpp); what these files share --
// SPARTA_GUARD_BEGIN / _END, CaptureScope, DeviceCall, open_call, timed_launches, device_call -- is in vbs_host.hpp.
#include "vbs_host.hpp"

using namespace sparta_dev;

namespace {

bool force_generic() { const char* e = std::getenv("SPARTA_FORCE_GENERIC"); return e && e[0] == '1'; }

// the refusal of an entry that writes values into a handle made without SPARTA_CREATE_UPDATABLE
int not_updatable(const char* entry) {
    return sparta::fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle was not made with SPARTA_CREATE_UPDATABLE (sparta_vbs_create_range_ex; handles of "
                                                                     "sparta_vbs_create_from_csr and sparta_vbs_create_transposed cannot take new values)");
}

// an environment switch that is on unless set to 0 (SPARTA_SGD_FUSE, SPARTA_ADAM_FUSE: read at every call, no plan depends on them)
bool env_switch(const char* name) {
    const char* e = std::getenv(name);
    return !e || atoi(e) != 0;
}

// every device array and event of the handle is a member that frees itself, with the handle's device current
void destroy_impl(sparta_vbs* v) {
    if (!v) return;
    DeviceGuard g(v->device);
    delete v;
}

// ---- the sparse-row leg of a handle on the host: no builder below makes a HIP call ----------------------------------------------------------------------
// 16-bit handles: the values the kernels multiply are the ROUNDED ones (a value that rounds to zero is a zero)
float stored_as(float x, int32_t dtype) {
    if (dtype == SPARTA_F32) return x;
    const bool bf16h = dtype == SPARTA_BF16;
    const uint16_t u = to_h16(x, bf16h);
    if (bf16h) { const uint32_t v32 = (uint32_t)u << 16; float f; std::memcpy(&f, &v32, 4); return f; }
    _Float16 hh; std::memcpy(&hh, &u, 2); return (float)hh;
}

// ---- sparse-row path: which block-rows are better served as rows of (column, value) --------------------------------
// An MFMA step (one <=32-row tile x 32 k x 128 columns) takes the time of ~12 nonzeros on the sparse-row path (2.1 ns per
// step across the 512 workers vs 512 B of B per nonzero and 128-column slab at ~3 TB/s): a block-row whose blocks hold
// fewer than SPARTA_SPARSE_K (default 24) nonzeros per step goes there (measured break-even, scripts/sparse_k_sweep.py:
// ~60 nonzeros per step while B fits the L2s, ~15 when its rows come from HBM).  SPARTA_SPARSE_K=0 switches the path off.
void collect_sparse_rows_from_ext(const sparta::HybridSparse& ext_, int64_t cols, int32_t dtype, SparseRowsHost& S) {
    const sparta::HybridSparse* ext = &ext_;
    std::vector<uint8_t>& sparse_flag = S.flag;
    std::vector<int64_t>& sp_rowptr = S.rowptr;
    std::vector<int32_t>&sp_col = S.col, &sp_crow = S.crow;
    std::vector<float>& sp_val = S.val;
    auto stored = [&](float x) -> float { return stored_as(x, dtype); };
    // flag 1: the block-row has no tile at all (skipped by the MFMA plans); flag 2 (mixed): its well-filled blocks are tiles like any other
    // (nzcount / jab hold only those), the nonzeros of its other blocks are sparse rows that ADD to C (bit 31 of their crow entry)
    sparse_flag.assign(ext->flag.size(), 0);
    bool any = false;
    // (flag 3: column-compacted tiles, UnionPlanHost -- no w-wide block either; their thinly used columns are sparse rows that add, as for flag 2)
    for (size_t q = 0; q < ext->flag.size(); q++) { sparse_flag[q] = ext->flag[q] == 1 || ext->flag[q] == 3; any = any || sparse_flag[q]; }
    if (!any) sparse_flag.clear();
    // the entries that survive the storage type (a value that rounds to zero is a zero) and lie inside the matrix: counted, then
    // copied, on all host threads (10^8..10^9 entries on the power-law configs)
    const int64_t n_ext = (int64_t)ext->crow.size();
    std::vector<int64_t> keep((size_t)n_ext + 1, 0);
    sparta::parallel_for_dynamic(n_ext, 2048, [&](int64_t lo, int64_t hi, int) {
        for (int64_t t = lo; t < hi; t++) {
            int64_t c = 0;
            for (int64_t k = ext->rowptr[(size_t)t]; k < ext->rowptr[(size_t)t + 1]; k++)
                c += stored(ext->val[(size_t)k]) != 0.0f && ext->col[(size_t)k] < cols;
            keep[(size_t)t + 1] = c;
        }
    });
    for (int64_t t = 0; t < n_ext; t++) keep[(size_t)t + 1] += keep[(size_t)t];
    sp_rowptr.swap(keep);
    sp_col.resize((size_t)sp_rowptr.back()); sp_val.resize((size_t)sp_rowptr.back()); sp_crow.resize((size_t)n_ext);
    sparta::parallel_for_dynamic(n_ext, 2048, [&](int64_t lo, int64_t hi, int) {
        for (int64_t t = lo; t < hi; t++) {
            int64_t o = sp_rowptr[(size_t)t];
            for (int64_t k = ext->rowptr[(size_t)t]; k < ext->rowptr[(size_t)t + 1]; k++) {
                const float a = stored(ext->val[(size_t)k]);
                if (a != 0.0f && ext->col[(size_t)k] < cols) { sp_col[(size_t)o] = ext->col[(size_t)k]; sp_val[(size_t)o] = a; o++; }
            }
            sp_crow[(size_t)t] = ext->crow[(size_t)t] | ((size_t)t < ext->row_add.size() && ext->row_add[(size_t)t] ? (int32_t)0x80000000 : 0);
        }
    });
}

void collect_sparse_rows_from_blocks(const StreamPlanIn& in, bool updatable, SparseRowsHost& S) {
    const int64_t cols = in.cols, w = in.w, br0 = in.br0, br1 = in.br1, jab_lo = in.jab_lo, mab_lo = in.mab_lo;
    const int64_t* row_part = in.row_part; const int64_t* nzcount = in.nzcount; const int64_t* jab = in.jab; const float* mab = in.mab;
    const bool h16 = in.dtype != SPARTA_F32;
    std::vector<uint8_t>& sparse_flag = S.flag;
    std::vector<int64_t>& sp_rowptr = S.rowptr;
    std::vector<int32_t>&sp_col = S.col, &sp_crow = S.crow;
    std::vector<float>& sp_val = S.val;
    auto stored = [&](float x) -> float { return stored_as(x, in.dtype); };
    double K = 24.0;
    if (const char* e = std::getenv("SPARTA_SPARSE_K")) K = atof(e);
    if (updatable) K = 0.0;          // (the sparse-row image holds only what was non-zero at creation: sparta_vbs_set_values could not fill it)
    if (K > 0.0) {
        sparse_flag.assign((size_t)(br1 - br0), 0);
        int64_t jo2 = 0, mo2 = 0, n_flagged = 0;
        const int64_t row0 = row_part[br0];
        std::vector<int64_t> cnt;
        sp_rowptr.push_back(0);
        // pass 1: which block-rows qualify and what they would cost as tiles (a handful stays with the tiles: see vbs_build_hybrid)
        std::vector<uint8_t> qualifies((size_t)(br1 - br0), 0);
        {
            double steps_saved = 0.0;
            int64_t mo1 = 0;
            for (int64_t ib = br0; ib < br1; ib++) {
                const int64_t h = row_part[ib + 1] - row_part[ib], nb = nzcount[ib];
                const float* blk = mab + mab_lo + mo1;
                const int64_t n_el = nb * h * w;
                int64_t nnz = 0;
                for (int64_t q = 0; q < n_el; q++) nnz += stored(blk[q]) != 0.0f;
                const int64_t kdep = h16 && w % 64 == 0 ? 64 : 32;                 // k depth of a step of the kernels this handle would use
                const double steps_br = (double)nb * (double)((w + kdep - 1) / kdep) * (double)((h + 31) / 32);
                if (h > 0 && nb > 0 && (double)nnz < K * steps_br) { qualifies[(size_t)(ib - br0)] = 1; steps_saved += steps_br; }
                mo1 += n_el;
            }
            if (steps_saved < (double)sparta::sparse_min_steps()) std::fill(qualifies.begin(), qualifies.end(), 0);
        }
        for (int64_t ib = br0; ib < br1; ib++) {
            const int64_t h = row_part[ib + 1] - row_part[ib], nb = nzcount[ib];
            const float* blk = mab + mab_lo + mo2;
            const int64_t n_el = nb * h * w;
            if (qualifies[(size_t)(ib - br0)] && (int64_t)sp_col.size() + n_el < ((int64_t)1 << 40)) {
                sparse_flag[(size_t)(ib - br0)] = 1;
                n_flagged++;
                // rows of this block-row: (column, value) in the reference's order (blocks ascending, k ascending: vbr.cpp:358-363)
                cnt.assign((size_t)h, 0);
                for (int64_t b = 0; b < nb; b++)
                    for (int64_t k = 0; k < w; k++)
                        for (int64_t i = 0; i < h; i++) cnt[(size_t)i] += (stored(blk[(b * w + k) * h + i]) != 0.0f) && jab[jab_lo + jo2 + b] * w + k < cols;
                const size_t base_row = sp_crow.size();
                for (int64_t i = 0; i < h; i++) {
                    sp_crow.push_back((int32_t)(row_part[ib] - row0 + i));
                    sp_rowptr.push_back(sp_rowptr.back() + cnt[(size_t)i]);
                }
                sp_col.resize((size_t)sp_rowptr.back());
                sp_val.resize((size_t)sp_rowptr.back());
                for (int64_t i = 0; i < h; i++) cnt[(size_t)i] = sp_rowptr[base_row + (size_t)i];
                for (int64_t b = 0; b < nb; b++) {
                    const int64_t c0 = jab[jab_lo + jo2 + b] * w;
                    for (int64_t k = 0; k < w && c0 + k < cols; k++)
                        for (int64_t i = 0; i < h; i++) {
                            const float a = stored(blk[(b * w + k) * h + i]);
                            if (a != 0.0f) { sp_col[(size_t)cnt[(size_t)i]] = (int32_t)(c0 + k); sp_val[(size_t)cnt[(size_t)i]++] = a; }
                        }
                }
            }
            jo2 += nb;
            mo2 += n_el;
        }
        if (n_flagged == 0) sparse_flag.clear();
    }
}

}  // namespace

namespace sparta_dev {

int order_sparse_rows(SparseRowsHost& S, int64_t cols) {
    std::vector<int64_t>& sp_rowptr = S.rowptr;
    std::vector<int32_t>&sp_col = S.col, &sp_crow = S.crow, &sp_list = S.list, &sp_stream_begin = S.stream_begin;
    std::vector<SpSegRec>& sp_segs = S.segs;
    std::vector<SpLongRec>& sp_long = S.longs;
    // a wave keeps SP_BATCH (16) rows of B in flight: a row of n nonzeros takes ~n / 16 memory latencies whatever else the GPU is doing, so rows
    // longer than kSpLong are cut into kSpSeg-nonzero segments that run on different waves (SPARTA_SPARSE_SEG overrides kSpSeg)
    // The segment length follows the size of the sparse part (decided below, once it is known): short segments keep a small
    // problem parallel (R-MAT 2^16: 128 -> 148 us, 512 -> 187 us), long ones save partial rows on a large one (2^20: 3.99 vs 3.75 ms).
    int64_t kSpSeg = 0;
    if (const char* e = std::getenv("SPARTA_SPARSE_SEG")) kSpSeg = std::max(8, atoi(e));
    // short rows: one wave each; rows with more than kSpLong nonzeros (hubs): segments of kSpSeg, one wave each + a reduction
    if (kSpSeg == 0) {
        const int64_t total = sp_rowptr.empty() ? 0 : sp_rowptr.back();
        // (below 1 M nonzeros the GPU has more idle waves than rows: 32-nonzero segments -- ca-HepPh: rows of up to 256 nonzeros on one wave each took
        // 57 us for 115 k nonzeros, 16 batches of gathers one after the other)
        kSpSeg = total < ((int64_t)1 << 20) ? 32 : (total < ((int64_t)4 << 20) ? 128 : (total < ((int64_t)16 << 20) ? 256 : 512));
    }
    int64_t kSpLong = 2 * kSpSeg;
    // Column windows.  The rows of B a launch gathers at any one time should lie close together: on a power-law matrix with millions of columns the nonzeros of the
    // rows in flight are spread over all of B (GBs), every gather is an HBM access (measured with FETCH_SIZE: 327 of 336 GB gathered came from HBM on a part of
    // the 8 M-row R-MAT) and the kernels run at the random-row rate of HBM.  So the columns are cut into windows of win_w columns (16-32 MB of B at N = 256..512
    // in 16 bits), a row of more than 128 nonzeros is cut into segments that also end where its columns cross into another window (once a segment holds sp_minseg
    // nonzeros), and the segments are PROCESSED window by window -- all rows' segments of window 0, then of window 1, ... (workgroups start in the order of the
    // list).  What is in flight then gathers from one window, which the Infinity Cache and the L2s hold: the same part 62.4 -> 35.1 ms, R-MAT 2^20 at 0.1 %
    // (B = 512, bf16) 11.6 -> 8.1 ms per part.  A row's partial rows are still added in segment order (the sum does not depend on the processing order).
    // Width / segment minimum 65536 / 64 -> 32768 / 128 (the defaults): another 3 % on both configs (34.8 -> 33.9 ms, 8.05 -> 7.80).
    // SPARTA_SP_WINDOW_COLS: unset = automatic (on from 262144 columns and 4 M nonzeros on this path), 0 = off, > 0 = the window width in columns;
    // SPARTA_SP_LONG / SPARTA_SP_MINSEG: the row length above which a row is cut / the nonzeros a segment holds before a window boundary ends it.
    const int64_t sp_total = sp_rowptr.empty() ? 0 : sp_rowptr.back();
    // Round 4: the windows are dealt to eight streams, one per XCD (below: every L2 then holds its OWN window instead of a copy of everybody's), and are 8192 columns wide
    // (2 MB of B per L2 at the 256-byte row chunks the large parts run with).  Parts of configs[4] / configs[3] at 1 %, sparse-row kernels, ms: one list of 32768-column
    // windows 25.8 / 31.5 / 10.7 -> eight streams of 8192-column windows 24.5 / 28.9 / 10.3 (4096 .. 32768 columns: within 1 %).  SPARTA_SP_XCD=0: one list, 32768 columns.
    bool sp_xcd = true;
    if (const char* e = std::getenv("SPARTA_SP_XCD")) sp_xcd = atoi(e) != 0;
    int64_t win_w = (cols >= 4 * 65536 && sp_total >= ((int64_t)4 << 20)) ? (sp_xcd ? 8192 : 32768) : 0, sp_minseg = 128;
    if (const char* e = std::getenv("SPARTA_SP_WINDOW_COLS")) win_w = std::max(0, atoi(e));
    if (win_w > 0) kSpLong = 128;
    if (const char* e = std::getenv("SPARTA_SP_LONG")) kSpLong = std::max(8, atoi(e));
    if (const char* e = std::getenv("SPARTA_SP_MINSEG")) sp_minseg = std::max(1, atoi(e));
    // the segments of row t (appended to out, or only counted when out is null)
    auto cut_row = [&](size_t t, std::vector<SpSegRec>* out) -> int32_t {
        const int64_t p0 = sp_rowptr[t], n = sp_rowptr[t + 1] - p0;
        int32_t n_seg = 0;
        if (win_w > 0) {
            const int64_t L = std::max<int64_t>(kSpSeg, 512);
            int64_t o = 0;
            while (o < n) {
                // the segment [o, e): up to L nonzeros, ending early at the first window boundary behind its first sp_minseg nonzeros
                int64_t e = std::min(n, o + L);
                if (e - o > sp_minseg) {
                    const int64_t wend = ((int64_t)sp_col[(size_t)(p0 + o + sp_minseg - 1)] / win_w + 1) * win_w;      // end of the window of the sp_minseg-th nonzero
                    const int32_t* b = sp_col.data() + p0 + o + sp_minseg;
                    const int32_t* bend = sp_col.data() + p0 + e;
                    const int32_t* f = std::lower_bound(b, bend, (int32_t)std::min<int64_t>(wend, INT32_MAX));
                    e = o + sp_minseg + (f - b);
                }
                if (out) out->push_back(SpSegRec{p0 + o, (int32_t)(e - o), 0});
                n_seg++;
                o = e;
            }
            return n_seg;
        }
        // a hub row's segments run in parallel, its partial rows are added one after the other: with segments of L nonzeros the chain is L / 16 gather
        // batches + n / L additions -- shortest near L = sqrt(1.6 n) (a batch ~ 10 additions), never below the size-dependent base, never above 512
        // (ia-wikiquote, 239 k nonzeros with rows of 10^4: 32-nonzero segments everywhere took 271 us, mostly the reduction of its hub rows)
        int64_t L = ((int64_t)std::sqrt(1.6 * (double)n) + 15) / 16 * 16;
        L = std::max(kSpSeg, std::min<int64_t>(512, L));
        for (int64_t o = 0; o < n; o += L) { if (out) out->push_back(SpSegRec{p0 + o, (int32_t)std::min<int64_t>(L, n - o), 0}); n_seg++; }
        return n_seg;
    };
    {
        // rows in order; the segments of the long ones are cut on all threads (chunks of rows, concatenated in row order)
        const int64_t n_rows_sp = (int64_t)sp_crow.size();
        const int nt = sparta::host_threads();
        const int64_t chunk = std::max<int64_t>(1024, (n_rows_sp + 4 * nt - 1) / (4 * std::max(nt, 1)));
        const int64_t n_chunks = (n_rows_sp + chunk - 1) / std::max<int64_t>(chunk, 1);
        std::vector<std::vector<SpSegRec>> segs_of((size_t)n_chunks);
        std::vector<std::vector<SpLongRec>> long_of((size_t)n_chunks);
        std::vector<std::vector<int32_t>> short_of((size_t)n_chunks);
        sparta::parallel_for_dynamic(n_chunks, 1, [&](int64_t lo, int64_t hi, int) {
            for (int64_t c = lo; c < hi; c++)
                for (int64_t t = c * chunk; t < std::min(n_rows_sp, (c + 1) * chunk); t++) {
                    if (sp_rowptr[(size_t)t + 1] - sp_rowptr[(size_t)t] <= kSpLong) { short_of[(size_t)c].push_back((int32_t)t); continue; }
                    SpLongRec lr{(int32_t)t, (int32_t)segs_of[(size_t)c].size(), 0, 0};      // seg_begin: within the chunk for now
                    lr.n_seg = cut_row((size_t)t, &segs_of[(size_t)c]);
                    long_of[(size_t)c].push_back(lr);
                }
        });
        for (int64_t c = 0; c < n_chunks; c++) {
            const int32_t base = (int32_t)sp_segs.size();
            if ((int64_t)sp_segs.size() + (int64_t)segs_of[(size_t)c].size() > INT32_MAX)
                return sparta::fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create: too many sparse-row segments for 32-bit indexing");
            sp_list.insert(sp_list.end(), short_of[(size_t)c].begin(), short_of[(size_t)c].end());
            sp_segs.insert(sp_segs.end(), segs_of[(size_t)c].begin(), segs_of[(size_t)c].end());
            for (SpLongRec lr : long_of[(size_t)c]) { lr.seg_begin += base; sp_long.push_back(lr); }
        }
    }
    // a segment's partial row lives at its index in row order (pad); the order of the list is the order the waves take them in: window by window
    // (a stable counting sort on the window of the segment's first column)
    for (size_t i = 0; i < sp_segs.size(); i++) sp_segs[i].pad = (int32_t)i;
    if (win_w > 0 && !sp_segs.empty()) {
        const int64_t n_win = (cols + win_w - 1) / win_w;
        std::vector<int64_t> start((size_t)n_win + 1, 0);
        for (const SpSegRec& g : sp_segs) start[(size_t)(sp_col[(size_t)g.p0] / win_w) + 1]++;
        for (int64_t k = 0; k < n_win; k++) start[(size_t)k + 1] += start[(size_t)k];
        std::vector<SpSegRec> sorted(sp_segs.size());
        for (const SpSegRec& g : sp_segs) sorted[(size_t)start[(size_t)(sp_col[(size_t)g.p0] / win_w)]++] = g;
        sp_segs.swap(sorted);
        // XCD-affine order (k_sparse.hip: sparse_segments_xcd_kernel): the windows are dealt to eight streams -- heaviest first, each to the stream with the fewest
        // nonzeros so far -- and the list becomes stream 0's windows in column order, then stream 1's, ...; workgroup b takes from stream b % 8 = its XCD.
        if (sp_xcd && sp_segs.size() >= 64) {
            std::vector<int64_t> w_nnz((size_t)n_win, 0), w_begin((size_t)n_win + 1, 0);
            for (const SpSegRec& g : sp_segs) { const size_t k = (size_t)(sp_col[(size_t)g.p0] / win_w); w_nnz[k] += g.cnt; w_begin[k + 1]++; }
            for (int64_t k = 0; k < n_win; k++) w_begin[(size_t)k + 1] += w_begin[(size_t)k];
            std::vector<int64_t> order((size_t)n_win);
            for (int64_t k = 0; k < n_win; k++) order[(size_t)k] = k;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return w_nnz[(size_t)a] > w_nnz[(size_t)b]; });
            int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            std::vector<int8_t> stream_of((size_t)n_win, 0);
            for (int64_t k : order) {
                int best = 0;
                for (int x = 1; x < 8; x++) if (load[x] < load[best]) best = x;
                stream_of[(size_t)k] = (int8_t)best;
                load[best] += w_nnz[(size_t)k] + 16 * (w_begin[(size_t)k + 1] - w_begin[(size_t)k]);       // (a segment costs about a batch whatever it holds)
            }
            std::vector<SpSegRec> streamed;
            streamed.reserve(sp_segs.size());
            sp_stream_begin.assign(9, 0);
            for (int x = 0; x < 8; x++) {
                sp_stream_begin[(size_t)x] = (int32_t)streamed.size();
                for (int64_t k = 0; k < n_win; k++)
                    if (stream_of[(size_t)k] == x) streamed.insert(streamed.end(), sp_segs.begin() + w_begin[(size_t)k], sp_segs.begin() + w_begin[(size_t)k + 1]);
            }
            sp_stream_begin[8] = (int32_t)streamed.size();
            sp_segs.swap(streamed);
        }
    }
    S.seg = kSpSeg; S.long_cut = kSpLong; S.minseg = sp_minseg; S.win_w = win_w;
    return SPARTA_OK;
}

// ---- resident-column product (k_colres.hip): A as length-sorted slots, 64 to a slice -----------------------------------------------------------
// Only for handles whose rows of C are ALL sparse rows (nothing for a tile launch to store first) and small enough that a column of B (and of C, with the
// extra cells of the long rows) fits LDS.  SPARTA_COLRES=0: never built.  SPARTA_COLRES_LMAX: longest slot (default max(32, nnz / 2048): at 1024 lanes per
// workgroup a slot of twice the average load per lane is not the critical path).
// force_parts > 1: that many parts of the rows of C (about equal staging images), one K range -- the image for products of few column sets
bool build_colres(int64_t rows, int64_t cols, const std::vector<int64_t>& rowptr, const std::vector<int32_t>& col, const std::vector<float>& val,
                  const std::vector<int32_t>& crow, ColresHost& H, int force_parts) {
    if (const char* e = std::getenv("SPARTA_COLRES")) if (atoi(e) == 0) return false;
    const int64_t n = (int64_t)crow.size(), nnz = rowptr.empty() ? 0 : rowptr.back();
    // The sparse rows may be SOME of the rows of C (the others belong to block-rows of MFMA tiles, whose launches come first and which this kernel leaves alone), and a sparse row may belong to
    // a MIXED block-row (bit 31 of crow: its well-filled blocks are tiles, this kernel ADDS the rest): H.mode says per row of C.  Not worth a second image and B / C through LDS for a
    // handful of sparse rows: at least half the rows.
    if (n > rows || 2 * n < rows || nnz == 0 || rows > kColresMaxParts * kColresCells || cols > kColresMaxRanges * (kColresCells - 8)) return false;
    std::vector<int32_t> ord_of((size_t)rows, -1);                                    // sparse row of every row of C (-1: none)
    H.mode.assign((size_t)((rows + 3) / 4 * 4), 0);                                    // 0: not this kernel's row, 1: store, 2: add to what the tile launches stored
    for (int64_t t = 0; t < n; t++) {
        const int32_t r = crow[(size_t)t] & 0x7fffffff;
        if (r >= rows || ord_of[(size_t)r] >= 0) return false;                         // not distinct rows of C
        ord_of[(size_t)r] = (int32_t)t;
        H.mode[(size_t)r] = crow[(size_t)t] < 0 ? 2 : 1;
    }
    int64_t lmax = std::max<int64_t>(32, nnz / 2048);
    if (const char* e = std::getenv("SPARTA_COLRES_LMAX")) lmax = std::max(1, atoi(e));
    constexpr int64_t kWaves = kColresWaves;
    // ---- K ranges: the rows of B a workgroup holds at a time (+ the zero cell), equal, multiples of 4 ----
    int64_t max_range = kColresCells - 8;
    if (const char* e = std::getenv("SPARTA_COLRES_RANGE")) max_range = std::max<int64_t>(64, std::min<int64_t>(max_range, atoi(e)) / 4 * 4);      // (tests: small matrices in several ranges)
    const int64_t n_ranges = (cols + max_range - 1) / max_range;
    if (n_ranges > kColresMaxRanges) return false;
    const int64_t range_len = ((cols + n_ranges - 1) / n_ranges + 3) / 4 * 4;
    H.krange.assign((size_t)n_ranges + 1, 0);
    for (int64_t r = 0; r <= n_ranges; r++) H.krange[(size_t)r] = (int32_t)std::min(cols, r * range_len);
    // ---- parts: contiguous ranges of the rows of C whose staging image (rows + the extra cells of their chunked rows) fits ----
    int64_t max_plane = kColresCells;
    if (const char* e = std::getenv("SPARTA_COLRES_PLANE")) max_plane = std::max<int64_t>(64, std::min<int64_t>(max_plane, atoi(e)) / 4 * 4);
    auto chunks_of = [&](int64_t r) -> int64_t {
        const int64_t t = ord_of[(size_t)r];
        if (t < 0) return 1;                                                           // (a row of another kernel: a cell of the staging image nobody writes or reads)
        return std::max<int64_t>(1, (rowptr[(size_t)t + 1] - rowptr[(size_t)t] + lmax - 1) / lmax);
    };
    if (force_parts > 1) {
        int64_t total_cells = 0;
        for (int64_t r = 0; r < rows; r++) total_cells += chunks_of(r);
        max_plane = std::min<int64_t>(max_plane, ((total_cells + force_parts - 1) / force_parts + 256 + 3) / 4 * 4);
    }
    std::vector<int64_t> part_begin{0};
    {
        int64_t cells = 0;
        for (int64_t r = 0; r < rows; r += 4) {                                       // (four rows at a time: every part starts at a multiple of 4 -- 16-byte stores of C)
            int64_t add = 4;
            for (int64_t q = r; q < std::min(rows, r + 4); q++) add += chunks_of(q) - 1;
            if (add > max_plane) return false;
            if (cells + add > max_plane) { part_begin.push_back(r); cells = 0; }
            cells += add;
        }
        part_begin.push_back(rows);
    }
    const int64_t n_parts = (int64_t)part_begin.size() - 1;
    if (n_parts > kColresMaxParts) return false;
    // Several parts / ranges are built only on request (SPARTA_COLRES_CUTS=1; tested, bit-identical to the uncut image): measured on the reference's two larger real matrices at N = 8192
    // they LOSE to the windowed row gather -- social_location (58 k x 58 k, 3.7 nonzeros per row: 2 parts x 2 ranges) 4.26 against 2.60 ms, ia-wikiquote (21.6 k x 94 k: 3 ranges) 3.25
    // against 2.75: one column per workgroup (4-byte LDS reads, A streamed N times), and rows of 2-4 nonzeros spread over the ranges pad every slice to a batch per range (3.3 x the nonzeros).
    {
        const char* e = std::getenv("SPARTA_COLRES_CUTS");
        if (force_parts > 1) { if (n_ranges != 1 || n_parts < 2) return false; }
        else if (n_parts * n_ranges > 1 && !(e && atoi(e) != 0)) return false;
    }
    bool unit = true;
    for (int64_t k = 0; k < nnz && unit; k++) unit = val[(size_t)k] == 1.0f;
    if (const char* e = std::getenv("SPARTA_COLRES_UNIT")) unit = unit && atoi(e) != 0;      // (0: keep the value array of a pattern matrix -- developer A/B)
    struct Slot { int64_t p0; int32_t len, dest; };
    int64_t total = 0;                                                                // batches so far (all parts, ranges, waves)
    struct Fill { int64_t batch0; int32_t wb; };                                      // where a (sorted slice, range) starts and how wide it is
    for (int64_t p = 0; p < n_parts; p++) {
        const int64_t r0 = part_begin[(size_t)p], r1 = part_begin[(size_t)p + 1], prow = r1 - r0, rows_pad = (prow + 3) / 4 * 4;
        std::vector<Slot> slots;
        const size_t longs0 = H.longs.size();
        int64_t n_extra = 0;
        for (int64_t r = r0; r < r1; r++) {
            const int64_t t = ord_of[(size_t)r];
            if (t < 0) continue;
            const int64_t p0 = rowptr[(size_t)t], len = rowptr[(size_t)t + 1] - p0, chunks = chunks_of(r);
            if (chunks > 1) H.longs.push_back(ColresLong{(int32_t)(r - r0), (int32_t)(rows_pad + n_extra), (int32_t)(chunks - 1), 0});
            for (int64_t c = 0; c < chunks; c++) {
                const int64_t o = c * lmax;
                slots.push_back(Slot{p0 + o, (int32_t)std::max<int64_t>(0, std::min<int64_t>(lmax, len - o)), c == 0 ? (int32_t)(r - r0) : (int32_t)(rows_pad + n_extra + c - 1)});
            }
            n_extra += chunks - 1;
        }
        const int64_t plane = (rows_pad + n_extra + 3) / 4 * 4;
        if (plane > kColresCells || (int64_t)slots.size() > (int64_t)colres_max_slices(1) * 64) return false;
        std::stable_sort(slots.begin(), slots.end(), [](const Slot& a, const Slot& b) { return a.len > b.len; });
        const int64_t n_slices = ((int64_t)slots.size() + 63) / 64;
        // where the entries of a slot fall into the K ranges
        std::vector<int32_t> cut((size_t)slots.size() * (size_t)(n_ranges + 1), 0);
        for (size_t q = 0; q < slots.size(); q++) {
            const int32_t* c0 = col.data() + slots[q].p0;
            for (int64_t r = 0; r <= n_ranges; r++)
                cut[q * (size_t)(n_ranges + 1) + (size_t)r] = (int32_t)(std::lower_bound(c0, c0 + slots[q].len, H.krange[(size_t)r]) - c0);
        }
        ColresPartDev pd;
        pd.r0 = (int32_t)r0; pd.rows = (int32_t)prow; pd.n_slices = (int32_t)n_slices; pd.n_long = (int32_t)(H.longs.size() - longs0); pd.plane = (int32_t)plane;
        pd.meta = (int32_t)H.meta.size(); pd.dest = (int32_t)H.dest.size(); pd.longs = (int32_t)longs0;
        pd.all_store = 1; pd.pad = 0;
        for (int64_t r = r0; r < r1; r++) if (H.mode[(size_t)r] != 1) pd.all_store = 0;
        const size_t m_wslice = H.meta.size(), m_woff = m_wslice + 17, m_bnd = m_woff + (size_t)n_ranges * 17;
        H.meta.resize(m_bnd + (size_t)n_ranges * (size_t)n_slices, 0);
        const size_t d0 = H.dest.size();
        H.dest.resize(d0 + (size_t)n_slices * 64, -1);
        // wave-major order: wave w owns the slices w, w + 16, ... of the sorted list (equally long streams)
        std::vector<int64_t> at_slice((size_t)n_slices, 0);
        {
            int64_t k_slice = 0;
            for (int64_t w = 0; w < kWaves; w++) {
                H.meta[m_wslice + (size_t)w] = (int32_t)k_slice;
                for (int64_t s = w; s < n_slices; s += kWaves) at_slice[(size_t)s] = k_slice++;
            }
            H.meta[m_wslice + (size_t)kWaves] = (int32_t)k_slice;
        }
        std::vector<Fill> fill((size_t)n_slices * (size_t)n_ranges);
        for (int64_t r = 0; r < n_ranges; r++) {
            for (int64_t w = 0; w < kWaves; w++) {
                H.meta[m_woff + (size_t)r * 17 + (size_t)w] = (int32_t)total;
                const int64_t first = total;
                for (int64_t s = w; s < n_slices; s += kWaves) {
                    int32_t longest = 0;
                    for (size_t q = (size_t)s * 64; q < std::min(slots.size(), (size_t)s * 64 + 64); q++)
                        longest = std::max(longest, cut[q * (size_t)(n_ranges + 1) + (size_t)r + 1] - cut[q * (size_t)(n_ranges + 1) + (size_t)r]);
                    const int32_t wb = std::max(1, (longest + 3) / 4);                  // never an empty slice: the kernel parks a slice's sums behind its last batch
                    fill[(size_t)s * (size_t)n_ranges + (size_t)r] = Fill{total, wb};
                    total += wb;
                    H.meta[m_bnd + (size_t)r * (size_t)n_slices + (size_t)at_slice[(size_t)s]] = (int32_t)(total - first);
                    if (total * 256 > (int64_t)INT32_MAX / 2) return false;
                }
            }
            H.meta[m_woff + (size_t)r * 17 + (size_t)kWaves] = (int32_t)total;
        }
        // the entries.  Past a slot's end in a range: the range's length -- one more cell of LDS, which the kernel clears -- with the value 0.0f: no per-lane condition, and nothing of B
        // is multiplied by a padding zero
        H.col.resize((size_t)(total + 1) * 256, 0);                                     // (+ one batch: a wave without slices still reads the first line of its empty stream)
        if (!unit) H.val.resize((size_t)(total + 1) * 256, 0.0f);
        for (int64_t s = 0; s < n_slices; s++) {
            for (int64_t r = 0; r < n_ranges; r++) {
                const Fill f = fill[(size_t)s * (size_t)n_ranges + (size_t)r];
                const uint16_t pad = (uint16_t)(H.krange[(size_t)r + 1] - H.krange[(size_t)r]);
                for (size_t x = (size_t)f.batch0 * 256; x < (size_t)(f.batch0 + f.wb) * 256; x++) H.col[x] = pad;
                for (int64_t l = 0; l < 64; l++) {
                    const size_t q = (size_t)s * 64 + (size_t)l;
                    if (q >= slots.size()) continue;
                    const int32_t b = cut[q * (size_t)(n_ranges + 1) + (size_t)r], e = cut[q * (size_t)(n_ranges + 1) + (size_t)r + 1];
                    for (int32_t k = b; k < e; k++) {
                        const size_t at = ((size_t)(f.batch0 + (k - b) / 4) * 64 + (size_t)l) * 4 + (size_t)((k - b) % 4);
                        H.col[at] = (uint16_t)(col[(size_t)(slots[q].p0 + k)] - H.krange[(size_t)r]);
                        if (!unit) H.val[at] = val[(size_t)(slots[q].p0 + k)];
                    }
                }
            }
        }
        for (size_t q = 0; q < slots.size(); q++) H.dest[d0 + (size_t)at_slice[q / 64] * 64 + q % 64] = slots[q].dest;
        H.parts.push_back(pd);
        H.max_slices = std::max(H.max_slices, (int32_t)n_slices);
        H.max_cells = std::max(H.max_cells, (int32_t)plane);
    }
    for (size_t x = (size_t)total * 256; x < H.col.size(); x++) H.col[x] = (uint16_t)(H.krange[1] - H.krange[0]);
    // a wave that owns no slice of a part (every part of fewer than 16 slices has such waves) still prefetches the destination cells of "its first slice" = one
    // slice behind the part's last (k_colres.hip: dst[I] = dest[(sl0 + ...) * 64 + lane]); behind the LAST part that is past the table: one padding slice of -1
    H.dest.resize(H.dest.size() + 64, -1);
    H.max_cells = std::max(H.max_cells, (int32_t)((range_len + 4) / 4 * 4));
    H.entries = total * 256;
    H.lmax = (int32_t)lmax;
    return true;
}

}  // namespace sparta_dev

namespace {

void build_colres_images(int64_t rows, int64_t cols, const SparseRowsHost& S, ColresImages& I) {
    I.has_main = build_colres(rows, cols, S.rowptr, S.col, S.val, S.crow, I.main);
    if (!I.has_main) return;
    // the four-part image for products of few column sets (SPARTA_COLRES_SMALL=0: not built)
    const char* es = std::getenv("SPARTA_COLRES_SMALL");
    if (I.main.parts.size() == 1 && I.main.krange.size() == 2 && rows >= 2048 && !(es && atoi(es) == 0))
        I.has_small = build_colres(rows, cols, S.rowptr, S.col, S.val, S.crow, I.small, 4) && I.small.val.empty() == I.main.val.empty();
}

// columns of B per workgroup: as many as LDS holds next to each other (columns of B first, the staging image of C after them, in the same cells)
// ... as many as fit: with one workgroup per CU the phases (columns of B in, stream of A, columns of C out) take the sum of their times, and the stream of A costs the same
// per workgroup whatever NC (measured): fewer passes win.  SPARTA_COLRES_NC caps it (read per call: developer A/B, tests).
int colres_columns(const sparta_vbs_t* A, int n_cols) {
    if (A->cr_slices == 0) return 0;
    const int64_t cells = A->cr_plane;                             // what a column set needs in LDS: the largest range of B (+ its zero cell) or the largest staging image
    const int fit = (int)std::min<int64_t>(std::min<int64_t>(4, kColresCells / cells), n_cols);
    int nc = fit;
    // (a product of fewer workgroups than CUs is ONE round whatever NC: the stream of A with three or four columns per cell costs twice the LDS time of one or two --
    // bcsstk18 at N = 128: 16.5 / 14.7 / 17.9 us with 1 / 2 / 3 columns)
    if (nc > 2 && (int64_t)((n_cols + 1) / 2) * A->cr_parts <= 256) nc = 2;             // (one round with two columns as well)
    else if (nc > 1) {
        // several rounds of workgroups: a round costs ~13 us + 3.4 us per column (measured per workgroup on the reference's real matrices: 16.5 / 18.7 / 23.4 / 27 us with 1..4
        // columns), and a last round is paid in full however few workgroups it has: N = 1024 on 256 CUs is 2 full rounds with two columns, 1.34 -> 2 with three
        // (bcsstk18 0.045 against 0.052 ms)
        int best = nc;
        double best_t = 1e300;
        for (int c = 1; c <= fit; c++) {
            const double rounds = std::ceil(std::ceil((double)n_cols / c) * A->cr_parts / 256.0), t = rounds * (13.0 + 3.4 * c);
            if (t <= best_t) { best_t = t; best = c; }
        }
        nc = best;
    }
    if (const char* e = std::getenv("SPARTA_COLRES_NC")) nc = std::min(fit, std::max(1, atoi(e)));
    while (nc > 1 && A->cr_slices > colres_max_slices(nc)) nc--;
    return nc >= 1 && A->cr_slices <= colres_max_slices(nc) ? nc : 0;
}

// ---- creation: per family a host builder (no HIP call; the stream and union plans are in vbs_plan.cpp / vbs_union.cpp) and an upload that copies its arrays to the device and fills in the handle's counters --------------------------------------
// a HIP call of an upload: out of device memory is SPARTA_ERR_ALLOC, anything else SPARTA_ERR_HIP (`fail` is sparta::fail in the function that uses it)
#define CREATE_TRY(expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);                              \
            return fail(e_ == hipErrorOutOfMemory ? SPARTA_ERR_ALLOC : SPARTA_ERR_HIP, m_);                  \
        }                                                                                                    \
    } while (0)

int no_device() { return sparta::fail(SPARTA_ERR_NO_DEVICE, "sparta_vbs_create: no HIP device visible (this path has no CPU fallback)"); }

// compute units of the device the plans are cut for.  Asked once per creation, by device index (no device has to be current): build_stream_plans wants the
// count whenever w is a multiple of 32 and build_union_plan for every union plan, which leaves few handles that would not need it
int device_cu_count(int32_t device) {
    hipDeviceProp_t pr;
    return hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
}

// the handle's block columns in 32 bits, every one checked against the matrix
int narrow_jab(const int64_t* jab, int64_t jab_lo, int64_t nblocks, int64_t block_cols, std::vector<int32_t>& jab32) {
    using sparta::fail;
    jab32.assign((size_t)std::max<int64_t>(nblocks, 1), 0);
    for (int64_t q = 0; q < nblocks; q++) {
        const int64_t jb = jab[jab_lo + q];
        if (jb < 0 || jb >= block_cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: jab entry out of range");
        jab32[(size_t)q] = (int32_t)jb;
    }
    return SPARTA_OK;
}

void build_class_tiles(const StreamPlanIn& in, ClassTilesHost& T) {
    const int64_t cols = in.cols, w = in.w, br0 = in.br0, br1 = in.br1, jab_lo = in.jab_lo, block_cols = (in.cols - 1) / in.w + 1;
    const int64_t* row_part = in.row_part; const int64_t* nzcount = in.nzcount; const int64_t* jab = in.jab;
    const uint8_t* skip = in.skip;
    std::vector<TileDesc>(&tiles)[4] = T.tiles;
    std::vector<BlockRowDesc>& brows = T.brows;
    int64_t(&n_real)[4] = T.n_real;
    int64_t& exec_area = T.exec_area;
    // ---- plan: row tiles per class -----------------------------------------------------------------
    {
        int64_t jo2 = 0, mo2 = 0;
        const int64_t row0 = row_part[br0];
        for (int64_t ib = br0; ib < br1; ib++) {
            const int64_t h = row_part[ib + 1] - row_part[ib];
            const int64_t nb = nzcount[ib];
            if (h > 0) {
                BlockRowDesc br{mo2, jo2, (int32_t)nb, (int32_t)h, (int32_t)(row_part[ib] - row0), 0};
                brows.push_back(br);
                int64_t r0 = skip && skip[ib - br0] ? h : 0;     // sparse-row block-rows get no tiles
                while (r0 < h) {
                    const int64_t rem = h - r0;
                    int cls;
                    int64_t mt;
                    if (rem > 32) { cls = 2; mt = std::min<int64_t>(rem, 64); }
                    else if (rem > 16) { cls = 1; mt = rem; }
                    else { cls = 0; mt = rem; }
                    const bool tail = (cols % w != 0) && nb > 0 && jab[jab_lo + jo2 + nb - 1] == block_cols - 1;
                    TileDesc t{mo2 + r0, jo2, (int32_t)nb, (int32_t)h, (int32_t)(row_part[ib] - row0 + r0),
                               (int32_t)mt | (tail ? TILE_TAIL : 0)};
                    tiles[cls].push_back(t);
                    const int64_t padded = cls == 0 ? 16 : ((mt + 31) / 32) * 32;
                    exec_area += padded * w * nb;
                    r0 += mt;
                }
            }
            jo2 += nb;
            mo2 += nb * h * w;
        }
    }

    // ---- schedule: per class, 8 contiguous chunks of ~equal cost (one per XCD: neighbouring block-rows gather the
    // same B panels, so they should share an L2), each chunk sorted by descending cost (the hardware hands workgroups
    // to free slots in blockIdx order => longest-processing-time-first per XCD), interleaved so that entry t is XCD
    // t % 8's (t / 8)-th item; short chunks are padded with empty tiles (nb = 0, mt = 0: nothing loaded or stored).
    for (int c = 0; c < 4; c++) n_real[c] = (int64_t)tiles[c].size();
    {
        const char* ord = std::getenv("SPARTA_TILE_ORDER");
        const bool natural = ord && std::strcmp(ord, "natural") == 0;
        for (int c = 0; c < 4; c++) {
            std::vector<TileDesc>& L = tiles[c];
            if (L.empty()) continue;
            const int64_t rows_pad = c == 0 ? 16 : (c == 1 ? 32 : 64);
            auto cost = [&](const TileDesc& t) { return (int64_t)t.nb * rows_pad + rows_pad / 4; };
            int64_t total = 0;
            for (const TileDesc& t : L) total += cost(t);
            std::vector<std::vector<TileDesc>> chunk(8);
            int64_t acc_cost = 0;
            for (const TileDesc& t : L) {
                int x = (int)std::min<int64_t>(7, (acc_cost * 8) / std::max<int64_t>(total, 1));
                chunk[(size_t)x].push_back(t);
                acc_cost += cost(t);
            }
            size_t maxlen = 0;
            for (auto& ch : chunk) {
                if (!natural) std::stable_sort(ch.begin(), ch.end(), [&](const TileDesc& a, const TileDesc& b) { return cost(a) > cost(b); });
                maxlen = std::max(maxlen, ch.size());
            }
            std::vector<TileDesc> arranged(maxlen * 8, TileDesc{0, 0, 0, 1, 0, 0});
            for (size_t x = 0; x < 8; x++)
                for (size_t j = 0; j < chunk[x].size(); j++) arranged[j * 8 + x] = chunk[x][j];
            L.swap(arranged);
        }
    }
}

// the device form of the column-compacted tiles of the hybrid builder
int build_union_host(const sparta::UnionPlanHost& uni, int32_t dtype, int n_cus, UnionDevPlan& uplan) {
    if (uni.empty()) return SPARTA_OK;
    // (workgroups per CU the kernel is built for: k_union.hip's launch bound and LDS; SPARTA_UNION_WPC: developer A/B)
    const int wpc = [] { const char* e = std::getenv("SPARTA_UNION_WPC"); return e ? std::max(1, atoi(e)) : 3; }();
    return build_union_plan(uni, wpc * n_cus, uplan, dtype, n_cus);
}

// the block-column index of sparta_vbs_spmm_t (pattern only) and, for 16-bit handles, the [ceil(h / 8)][w][8] image of k_spmm_t.hip; fp32 handles read d_A (kept: drop_legacy_image)
int build_spmm_t_host(const StreamPlanIn& in, SpmmTHost& H) {
    const bool h16 = in.dtype != SPARTA_F32, bf16h = in.dtype == SPARTA_BF16;
    const int64_t w = in.w, mab_lo = in.mab_lo;
    const float* mab = in.mab;
    SpmmTIndexHost& T = H.index;
    if (int rc = build_spmm_t_index(in.cols, w, in.br0, in.br1, in.row_part, in.nzcount, in.jab, in.jab_lo, h16, T)) return rc;
    if (h16 && T.image_elems > 0) {
        std::unique_ptr<uint16_t[]>& img = H.image;
        img.reset(new uint16_t[(size_t)T.image_elems]);
        sparta::parallel_for_dynamic((int64_t)T.src.size(), 64, [&](int64_t lo, int64_t hi, int) {
            for (int64_t q = lo; q < hi; q++) pack_spmm_t_block(mab + mab_lo + T.src[(size_t)q].src, T.src[(size_t)q].h, w, bf16h, img.get() + T.src[(size_t)q].dst);
        });
    }
    return SPARTA_OK;
}

// A itself: the caller's blocks (fp32), or the 16-bit slices of the stream plans with the sources of an updatable handle's slices
int upload_a_image(sparta_vbs* v, const StreamPlanIn& in, bool updatable, const StreamPlanHost& plan) {
    using sparta::fail;
    const bool h16 = in.dtype != SPARTA_F32;
    const int64_t nztot = v->nztot, mab_lo = in.mab_lo, kp = plan.kp;
    const float* mab = in.mab;
    // A is padded by 128 floats so that no (masked-off) lane ever forms an address past the allocation
    if (!h16) {
        v->a_bytes = (nztot + 128) * (int64_t)sizeof(float);
        CREATE_TRY(v->d_A.upload(nztot > 0 ? mab + mab_lo : nullptr, (size_t)nztot, 128));
    } else {
        // the look-ahead of the pipeline reads up to 5 slices past the last one (never multiplied): pad
        const std::vector<uint16_t>& a0 = plan.a16_steps[0];
        const std::vector<uint16_t>& a1 = plan.a16_steps[1];
        v->a_bytes = ((int64_t)a0.size() + (int64_t)a1.size() + 8 * 64 * 64) * (int64_t)sizeof(uint16_t);
        CREATE_TRY(v->d_A.alloc(0, (size_t)v->a_bytes));
        CREATE_TRY(hipMemset(v->d_A, 0, (size_t)v->a_bytes));
        if (!a0.empty()) CREATE_TRY(hipMemcpy(v->d_A, a0.data(), a0.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        if (!a1.empty()) CREATE_TRY(hipMemcpy((uint16_t*)v->d_A.get() + a0.size(), a1.data(), a1.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        v->kp16 = (int)kp;
        v->upd_base[1] = (int64_t)a0.size();
        for (int ty = 0; ty < 2 && updatable; ty++) {
            if (plan.upd_map[ty].empty()) continue;
            for (const UpdSlice& u : plan.upd_map[ty]) v->upd_cover[ty] += (int64_t)(u.rows_lo + u.rows_hi) * kp;
            CREATE_TRY(v->d_upd_map[ty].upload(plan.upd_map[ty]));
        }
        if (updatable && !plan.upd_hub.empty()) {
            v->n_upd_hub = (int64_t)plan.upd_hub.size();
            CREATE_TRY(v->d_upd_hub.upload(plan.upd_hub));
        }
    }
    return SPARTA_OK;
}

int upload_class_tiles(sparta_vbs* v, const std::vector<int32_t>& jab32, const ClassTilesHost& T) {
    using sparta::fail;
    const std::vector<TileDesc>(&tiles)[4] = T.tiles;
    const std::vector<BlockRowDesc>& brows = T.brows;
    const int64_t(&n_real)[4] = T.n_real;
    v->exec_area = T.exec_area;
    CREATE_TRY(v->d_jab.upload(jab32));
    for (int c = 0; c < 4; c++) {
        v->n_tiles[c] = (int64_t)tiles[c].size();
        v->n_real_tiles[c] = n_real[c];
        if (tiles[c].empty()) continue;
        CREATE_TRY(v->d_tiles[c].upload(tiles[c]));
    }
    v->n_brows = (int64_t)brows.size();
    if (!brows.empty()) CREATE_TRY(v->d_brows.upload(brows));
    return SPARTA_OK;
}

// the stream plans: step lists (padded here), worker ranges, fix-up records, the fragment / packed image of fp32 one-tile plans, the hub plan
int upload_stream_plans(sparta_vbs* v, const StreamPlanIn& in, bool updatable, StreamPlanHost& plan) {
    using sparta::fail;
    const bool h16 = in.dtype != SPARTA_F32;
    const int64_t cols = in.cols, w = in.w;
    v->zero_ranges = plan.zero_ranges;
    std::vector<StepRec>(&steps)[2] = plan.steps;
    std::vector<int32_t>(&wrange)[2] = plan.wrange;
    std::vector<FixRec>& fix = plan.fix;
    std::vector<int32_t>& fix_slots = plan.fix_slots;
    const int n_workers = plan.n_workers, n_split = plan.n_split;
    if (!steps[0].empty() || !steps[1].empty() || !fix.empty() || !plan.zero_ranges.empty() || plan.n_hub_steps > 0) {
        v->has_tail = (cols % w) != 0;
        v->n_workers = n_workers; v->n_fix = (int32_t)fix.size(); v->n_split = n_split; v->n_slots = (int32_t)fix_slots.size();
        std::vector<int32_t> big_fix;
        for (size_t q = 0; q < fix.size(); q++) {
            v->max_tile_slots = std::max(v->max_tile_slots, fix[q].n_slots);
            if (fix[q].n_slots > 2 * kFixGroup) big_fix.push_back((int32_t)q);
        }
        v->n_big_fix = (int32_t)big_fix.size();
        if (!big_fix.empty()) CREATE_TRY(v->d_big_fix.upload(big_fix));
        for (int ty = 0; ty < 2; ty++) {
            std::vector<StepRec>& st = steps[ty];
            v->n_steps[ty] = (int64_t)st.size();
            if (st.empty()) continue;
            if (updatable && !h16) for (const StepRec& r : st) v->upd_cover[ty] += (int64_t)(r.mt_flags & 0xffff) * SK_KP;
            // the pipeline prefetches up to 5 steps (and up to two 8-record batches) past a range end: pad with harmless copies
            for (int k = 0; k < 32; k++) { StepRec d = st[(size_t)v->n_steps[ty] - 1]; d.mt_flags = (d.mt_flags & ~(STEP_LAST | STEP_SPLIT)) | STEP_FIRST; st.push_back(d); }
            CREATE_TRY(v->d_steps[ty].upload(st));
            v->h_steps[ty] = st;
            v->n_plan_tiles[ty] = plan.n_plan_tiles[ty];
            v->tiles_row_aligned[ty] = plan.tiles_row_aligned[ty];
            if (ty == 0) v->wide16 = plan.wide16;
            CREATE_TRY(v->d_wrange[ty].upload(wrange[ty]));
        }
        if (!plan.a_frag.empty()) {
            // a SECOND copy of the one-tile part of A (4 KB per step whatever the tile height): if the device cannot hold it the handle is still
            // good -- d_a_frag stays null and the launch code runs the LDS-staged kernel on the legacy image (launch_f32_stream)
            if (v->d_a_frag.alloc(plan.a_frag.size()) == hipSuccess) {
                CREATE_TRY(hipMemcpy(v->d_a_frag, plan.a_frag.data(), plan.a_frag.size() * sizeof(float), hipMemcpyHostToDevice));
                v->a_bytes += (int64_t)(plan.a_frag.size() * sizeof(float));    // the device image holds the one-tile part of A twice (two layouts)
            } else {
                (void)hipGetLastError();
            }
        }
        if (!plan.a_pack.empty()) {
            // packed handles: the packed image INSTEAD of the fragment image, its step list and worker ranges, and the place of every block in it (for the rebuild
            // of the reference-layout image).  As above, a device that cannot hold the image leaves a handle that runs the LDS-staged kernel.
            std::vector<StepRec>& ps = plan.psteps;
            v->n_psteps = (int64_t)ps.size(); v->pack_slots = plan.pack_slots;
            for (int k = 0; k < 32; k++) { StepRec d = ps[(size_t)v->n_psteps - 1]; d.mt_flags = (d.mt_flags & ~(STEP_LAST | STEP_SPLIT)) | STEP_FIRST; ps.push_back(d); }
            if (v->d_a_pack.alloc(plan.a_pack.size()) == hipSuccess) {
                CREATE_TRY(hipMemcpy(v->d_a_pack, plan.a_pack.data(), plan.a_pack.size() * sizeof(float), hipMemcpyHostToDevice));
                v->a_bytes += (int64_t)(plan.a_pack.size() * sizeof(float));
                CREATE_TRY(v->d_psteps.upload(ps));
                CREATE_TRY(v->d_pwrange.upload(plan.pwrange));
                CREATE_TRY(v->d_pack_loc.upload(plan.pack_loc));
            } else {
                (void)hipGetLastError();
                v->n_psteps = 0; v->pack_slots = 0;
            }
        }
        if (plan.n_hub_steps > 0) {
            v->hub_g = plan.hub_g; v->hub_workers = plan.hub_workers; v->n_hub_steps = plan.n_hub_steps; v->hub_area = plan.hub_area;
            v->hub_union_area = plan.hub_union_area; v->n_hub_tiles = plan.n_hub_tiles; v->n_hub_groups = plan.n_hub_groups;
            v->hub_chunks = plan.hub_chunks; v->hub_segments = plan.hub_segments;
            CREATE_TRY(v->d_hub_steps.upload(plan.hub_steps));
            CREATE_TRY(v->d_hub_tiles.upload(plan.hub_tiles));
            CREATE_TRY(v->d_hub_wrange.upload(plan.hub_wrange));
            const size_t a_elems = plan.hub_a16_elems;
            CREATE_TRY(v->d_hub_A.upload(plan.hub_a16.get(), a_elems, 64));
            v->a_bytes += (int64_t)(a_elems * sizeof(uint16_t));
            v->exec_area += plan.hub_union_area;
            v->h_hub_steps.swap(plan.hub_steps);
        }
        if (!fix.empty()) CREATE_TRY(v->d_fix.upload(fix));
        CREATE_TRY(v->d_fix_slots.alloc(std::max<size_t>(fix_slots.size(), 1)));
        if (!fix_slots.empty()) CREATE_TRY(hipMemcpy(v->d_fix_slots, fix_slots.data(), fix_slots.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return SPARTA_OK;
}

int upload_union(sparta_vbs* v, const UnionDevPlan& uplan, const sparta::HybridSparse* ext) {
    using sparta::fail;
    const bool h16 = v->dtype != SPARTA_F32;
    for (int ty = 0; ty < kUnionTypes; ty++) {
        if (uplan.n_steps[ty] == 0) continue;
        v->u_workers[ty] = uplan.n_workers[ty]; v->u_steps[ty] = uplan.n_steps[ty]; v->u_tiles[ty] = uplan.n_tiles[ty]; v->u_steps_total += uplan.n_steps[ty];
        CREATE_TRY(v->d_u_rec[ty].upload(uplan.rec[ty]));
        CREATE_TRY(v->d_u_ids[ty].upload(uplan.ids[ty]));
        const size_t a_bytes_ty = h16 ? uplan.a16[ty].size() * sizeof(uint16_t) : uplan.a[ty].size() * sizeof(float);
        CREATE_TRY(v->d_u_a[ty].upload(h16 ? (const uint8_t*)uplan.a16[ty].data() : (const uint8_t*)uplan.a[ty].data(), a_bytes_ty));
        CREATE_TRY(v->d_u_wrange[ty].upload(uplan.wrange[ty]));
        CREATE_TRY(v->d_u_tail[ty].upload(uplan.tail[ty]));
        v->a_bytes += (int64_t)(a_bytes_ty + uplan.ids[ty].size() * sizeof(int32_t) + uplan.tail[ty].size() * sizeof(uint32_t));
        v->exec_area += uplan.n_steps[ty] * 32 * uplan.type_rows[ty];
        v->u_exec_area += uplan.n_steps[ty] * 32 * uplan.type_rows[ty];
    }
    v->u_area = uplan.area; v->u_cols = uplan.cols; v->u_nnz = ext->uni.nnz; v->u_tail_nnz = ext->uni.tail_nnz; v->u_rows = uplan.rows;
    for (int hh = 0; hh < 2; hh++) { v->u_tiles_h[hh] = uplan.tiles_by_height[hh]; v->u_steps_h[hh] = uplan.steps_by_height[hh]; }
    return SPARTA_OK;
}

int upload_sparse_rows(sparta_vbs* v, const SparseRowsHost& S) {
    using sparta::fail;
    const std::vector<int64_t>& sp_rowptr = S.rowptr;
    const std::vector<int32_t>&sp_col = S.col, &sp_crow = S.crow, &sp_list = S.list, &sp_stream_begin = S.stream_begin;
    const std::vector<float>& sp_val = S.val;
    const std::vector<SpSegRec>& sp_segs = S.segs;
    const std::vector<SpLongRec>& sp_long = S.longs;
    const int64_t n_sp_short = (int64_t)sp_list.size(), n_sp_long = (int64_t)sp_long.size();
    if (sp_crow.empty()) return SPARTA_OK;
    v->n_sp_rows = (int64_t)sp_crow.size(); v->n_sp_short = n_sp_short; v->n_sp_long = n_sp_long; v->sp_nnz = sp_rowptr.back();
    CREATE_TRY(v->d_sp_rowptr.upload(sp_rowptr));
    CREATE_TRY(v->d_sp_col.upload(sp_col, 64));      // +64: a batch reads up to SP_BATCH entries at once
    CREATE_TRY(v->d_sp_val.upload(sp_val, 64));
    CREATE_TRY(v->d_sp_crow.upload(sp_crow));
    if (!sp_list.empty()) CREATE_TRY(v->d_sp_list.upload(sp_list));
    if (!sp_long.empty()) {
        v->n_sp_segs = (int64_t)sp_segs.size();
        CREATE_TRY(v->d_sp_segs.upload(sp_segs));
        if (!sp_stream_begin.empty()) {
            CREATE_TRY(v->d_sp_stream_begin.upload(sp_stream_begin.data(), 9));
            for (int x = 0; x < 8; x++) v->sp_max_stream = std::max<int64_t>(v->sp_max_stream, sp_stream_begin[(size_t)x + 1] - sp_stream_begin[(size_t)x]);
        }
        CREATE_TRY(v->d_sp_long.upload(sp_long));
    }
    return SPARTA_OK;
}

int upload_colres(sparta_vbs* v, const ColresImages& I) {
    using sparta::fail;
    if (!I.has_main) return SPARTA_OK;
    const ColresHost& H = I.main;
    CREATE_TRY(v->d_cr_col.upload(H.col));
    if (!H.val.empty()) CREATE_TRY(v->d_cr_val.upload(H.val));
    CREATE_TRY(v->d_cr_meta.upload(H.meta));
    CREATE_TRY(v->d_cr_mode.upload(H.mode));
    CREATE_TRY(v->d_cr_parts.upload(H.parts));
    CREATE_TRY(v->d_cr_dest.upload(H.dest));
    if (!H.longs.empty()) CREATE_TRY(v->d_cr_longs.upload(H.longs));
    v->cr_slices = H.max_slices; v->cr_long = (int32_t)H.longs.size(); v->cr_plane = H.max_cells; v->cr_lmax = H.lmax;
    v->cr_parts = (int32_t)H.parts.size(); v->cr_ranges = (int32_t)H.krange.size() - 1;
    for (size_t r = 0; r < H.krange.size(); r++) v->cr_krange[r] = H.krange[r];
    v->cr_entries = H.entries;
    v->a_bytes += (int64_t)(H.col.size() * sizeof(uint16_t) + H.val.size() * sizeof(float));
    v->cr_unit = H.val.empty();
    if (!I.has_small) return SPARTA_OK;
    const ColresHost& S = I.small;
    auto& cs = v->cr_small;
    CREATE_TRY(cs.col.upload(S.col));
    if (!S.val.empty()) CREATE_TRY(cs.val.upload(S.val));
    CREATE_TRY(cs.meta.upload(S.meta));
    CREATE_TRY(cs.dest.upload(S.dest));
    if (!S.longs.empty()) CREATE_TRY(cs.longs.upload(S.longs));
    CREATE_TRY(cs.parts.upload(S.parts));
    cs.slices = S.max_slices; cs.plane = S.max_cells; cs.n_parts = (int32_t)S.parts.size();
    v->a_bytes += (int64_t)(S.col.size() * sizeof(uint16_t) + S.val.size() * sizeof(float));
    return SPARTA_OK;
}

int upload_spmm_t(sparta_vbs* v, const SpmmTHost& H, bool updatable) {
    using sparta::fail;
    const SpmmTIndexHost& T = H.index;
    v->n_t_items = (int64_t)T.items.size();
    v->n_t_blocks = (int64_t)T.blocks.size();
    CREATE_TRY(v->d_t_items.upload(T.items));
    if (!T.blocks.empty()) CREATE_TRY(v->d_t_blocks.upload(T.blocks));
    if (H.image) {
        const std::unique_ptr<uint16_t[]>& img = H.image;
        CREATE_TRY(v->d_t_A.upload(img.get(), (size_t)T.image_elems));
        v->a_bytes += T.image_elems * (int64_t)sizeof(uint16_t);
        if (updatable) {
            v->n_t_src = (int64_t)T.src.size();
            CREATE_TRY(v->d_t_src.upload(T.src));
        }
    }
    return SPARTA_OK;
}

// SPARTA_PLAN_DEBUG on a host without a GPU (developer aid, scripts/asan_host.sh): the host planning of the tiles runs to its end, then the call fails as usual
int plan_without_device(const StreamPlanIn& in, const sparta::HybridSparse* ext, sparta::BuildTrace& trace) {
    ClassTilesHost ct;
    build_class_tiles(in, ct);
    trace.lap("tile lists");
    StreamPlanHost plan;
    if (int rc = build_stream_plans(in, plan)) return rc;
    trace.lap("stream plans");
    UnionDevPlan uplan;
    if (ext) if (int rc = build_union_host(ext->uni, in.dtype, in.n_cus, uplan)) return rc;
    if (ext && !ext->uni.empty()) trace.lap("column-compacted tiles (plan)");
    return no_device();
}

}  // namespace

extern "C" {

int sparta_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// `ext` (sparta_vbs_create_from_csr): the sparse-row part of the matrix decided and collected by the hybrid host builder.  Fully sparse
// block-rows (ext->flag 1) have nzcount = 0 in the arrays given here and get neither tiles nor zero-fill records; MIXED block-rows (flag 2)
// keep their well-filled blocks in nzcount / jab / mab as tiles like any other, and the nonzeros of their other blocks are sparse rows that
// add to C behind the tile launches (see the ordering note at the sparse-row launch in spmm_impl).
static int create_core(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part,
                       const int64_t* nzcount, const int64_t* jab, const float* mab, int64_t br0, int64_t br1, int32_t dtype,
                       int32_t device, const sparta::HybridSparse* ext, int32_t flags = 0) {
    using sparta::fail;
    if (!out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: out is NULL");
    if (flags & ~(SPARTA_CREATE_UPDATABLE | SPARTA_CREATE_TRANSPOSE)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_range_ex: unknown bits in flags");
    const bool updatable = (flags & SPARTA_CREATE_UPDATABLE) != 0;        // every block-row stays in the dense-block images; the slices' sources are kept
    const bool transposable = (flags & SPARTA_CREATE_TRANSPOSE) != 0;     // sparta_vbs_spmm_t: block-column index + an image it can read (changes nothing of the forward product)
    if (transposable && ext) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create: SPARTA_CREATE_TRANSPOSE needs the dense blocks of every block-row");
    *out = nullptr;
    sparta::BuildTrace trace("vbs_create");
    if (rows <= 0 || cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: bad dimensions or NULL index array");
    if (br0 < 0 || br1 > block_rows || br0 >= br1) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: bad block-row range");
    if (dtype != SPARTA_F32 && dtype != SPARTA_F16 && dtype != SPARTA_BF16) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: bad dtype");
    const bool h16 = dtype != SPARTA_F32;
    if (h16 && w % 32 != 0)
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create: SPARTA_F16 / SPARTA_BF16 need block_col_size % 32 == 0 (only the stream kernels have a 16-bit form)");
    if (rows > INT32_MAX || w > (1 << 20)) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create: rows >= 2^31 or w > 2^20");
    const int64_t block_cols = (cols - 1) / w + 1;

    // validate the partition and locate the range inside jab / mab
    if (row_part[0] != 0 || row_part[block_rows] != rows) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: row_part must span [0, rows]");
    int64_t jab_lo = 0, mab_lo = 0, jab_hi = 0, mab_hi = 0, jo = 0, mo = 0;
    for (int64_t ib = 0; ib < block_rows; ib++) {
        const int64_t h = row_part[ib + 1] - row_part[ib];
        if (h < 0 || nzcount[ib] < 0 || nzcount[ib] > block_cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: invalid row_part / nzcount");
        if (h > INT32_MAX / 2 || nzcount[ib] > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create: block-row too large");
        if (ib == br0) { jab_lo = jo; mab_lo = mo; }
        jo += nzcount[ib];
        mo += nzcount[ib] * h * w;
        if (ib == br1 - 1) { jab_hi = jo; mab_hi = mo; }
    }
    const int64_t nblocks = jab_hi - jab_lo, nztot = mab_hi - mab_lo;
    if (nblocks > 0 && (!jab || !mab)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: jab / mab is NULL");

    const int ndev = sparta_device_count();
    const bool plan_debug = std::getenv("SPARTA_PLAN_DEBUG") != nullptr && ndev <= 0;   // developer aid: the host planning on a host without a GPU, then fail as usual
    if (ndev <= 0 && !plan_debug) return no_device();
    if (!plan_debug && (device < 0 || device >= ndev)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create: device index out of range");
    StreamPlanIn in{cols, w, br0, br1, jab_lo, mab_lo, row_part, nzcount, jab, mab, dtype, plan_debug ? 256 : device_cu_count(device), nullptr, updatable && h16, !h16 && flags == 0};
    std::vector<int32_t> jab32;
    if (int rc = narrow_jab(jab, jab_lo, nblocks, block_cols, jab32)) return rc;

    // ---- sparse rows: which block-rows are better served as rows of (column, value), and their device form; they live until the resident-column image is made ----
    SparseRowsHost sp;
    if (ext) collect_sparse_rows_from_ext(*ext, cols, dtype, sp);
    else collect_sparse_rows_from_blocks(in, updatable, sp);
    if (int rc = order_sparse_rows(sp, cols)) return rc;
    trace.lap("sparse rows (device form)");
    in.skip = sp.flag.empty() ? nullptr : sp.flag.data();
    if (plan_debug) return plan_without_device(in, ext, trace);

    // the handle is owned by `hold` until it is handed to the caller: any early return or exception below frees it and every
    // device allocation made so far
    struct VbsDeleter { void operator()(sparta_vbs* q) const { destroy_impl(q); } };
    std::unique_ptr<sparta_vbs, VbsDeleter> hold(new (std::nothrow) sparta_vbs);
    sparta_vbs* v = hold.get();
    if (!v) return fail(SPARTA_ERR_ALLOC, "sparta_vbs_create: out of host memory");
    v->device = device; v->dtype = dtype; v->create_flags = flags;
    v->rows = row_part[br1] - row_part[br0]; v->cols = cols; v->block_rows = br1 - br0; v->w = w;
    v->nblocks = nblocks; v->nztot = nztot;
    v->h_row_part.resize((size_t)(br1 - br0) + 1);          // what the block table of sparta_vbs_block_ssq / _mask_blocks is built from (with the handle's jab)
    for (int64_t ib = br0; ib <= br1; ib++) v->h_row_part[(size_t)(ib - br0)] = row_part[ib] - row_part[br0];
    v->h_nzcount.assign(nzcount + br0, nzcount + br1);

    DeviceGuard guard(device);
    if (!guard.ok) return fail(SPARTA_ERR_HIP, "sparta_vbs_create: hipSetDevice failed");
    {   // ---- the w-wide tiles: class tile lists and stream plans, with A's own image ----
        ClassTilesHost ct;
        build_class_tiles(in, ct);
        trace.lap("tile lists");
        StreamPlanHost plan;
        if (int rc = build_stream_plans(in, plan)) return rc;
        trace.lap("stream plans");
        if (int rc = upload_a_image(v, in, updatable, plan)) return rc;
        if (int rc = upload_class_tiles(v, jab32, ct)) return rc;
        if (int rc = upload_stream_plans(v, in, updatable, plan)) return rc;
    }
    if (ext) {   // ---- column-compacted tiles ----
        UnionDevPlan uplan;
        if (int rc = build_union_host(ext->uni, dtype, in.n_cus, uplan)) return rc;
        if (!ext->uni.empty()) trace.lap("column-compacted tiles (plan)");
        if (int rc = upload_union(v, uplan, ext)) return rc;
    }
    if (int rc = upload_sparse_rows(v, sp)) return rc;
    // resident-column image (k_colres.hip): at least half the rows of C are sparse rows (the tile launches, if any, come first on the stream), a column of B fits LDS
    if (!h16 && !sp.crow.empty()) {
        ColresImages cr;
        build_colres_images(v->rows, cols, sp, cr);
        if (int rc = upload_colres(v, cr)) return rc;
    }
    if (transposable) {
        SpmmTHost t;
        if (int rc = build_spmm_t_host(in, t)) return rc;
        if (int rc = upload_spmm_t(v, t, updatable)) return rc;
    }
    CREATE_TRY(v->ev0.create());
    CREATE_TRY(v->ev1.create());
    CREATE_TRY(v->tev0.create());
    CREATE_TRY(v->tev1.create());
    trace.lap("upload");
    *out = hold.release();
    return SPARTA_OK;
}

int sparta_vbs_create_range_ex(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part,
                               const int64_t* nzcount, const int64_t* jab, const float* mab, int64_t br0, int64_t br1, int32_t dtype,
                               int32_t device, int32_t flags) {
    SPARTA_GUARD_BEGIN
    const int rc = create_core(out, rows, cols, block_rows, w, row_part, nzcount, jab, mab, br0, br1, dtype, device, nullptr, flags);
    if (rc == SPARTA_OK) (*out)->from_vbs_arrays = true;      // (its blocks are the caller's blocks: sparta_vbs_block_ssq / sparta_vbs_mask_blocks)
    return rc;
    SPARTA_GUARD_END("sparta_vbs_create")
}

int sparta_vbs_create_range(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part,
                            const int64_t* nzcount, const int64_t* jab, const float* mab, int64_t br0, int64_t br1, int32_t dtype,
                            int32_t device) {
    return sparta_vbs_create_range_ex(out, rows, cols, block_rows, w, row_part, nzcount, jab, mab, br0, br1, dtype, device, 0);
}

static int create_from_csr_impl(sparta_vbs_t** out, int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                                const int64_t* grouping, int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size,
                                int32_t dtype, int32_t device, bool keep_order) {
    using sparta::fail;
    if (!out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_from_csr: out is NULL");
    *out = nullptr;
    if (dtype != SPARTA_F32 && dtype != SPARTA_F16 && dtype != SPARTA_BF16) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_from_csr: bad dtype");
    sparta_vbs_host h;
    std::memset(&h, 0, sizeof(h));
    int rc = SPARTA_OK;
    try {
        sparta::CsrView a;
        a.rows = rows; a.cols = cols; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
        double K = 24.0;
        if (const char* e = std::getenv("SPARTA_SPARSE_K")) K = atof(e);
        const int64_t kdep = (dtype != SPARTA_F32 && col_block_size % 64 == 0) ? 64 : 32;
        sparta::HybridSparse sp;
        sp.esz = dtype == SPARTA_F32 ? 4.0 : 2.0;
        sp.want_union = true;                                              // column-compacted tiles (k_union.hip: fp32 and 16-bit forms)
        sp.union_gran = dtype == SPARTA_F32 ? 16 : 32;
        rc = sparta::vbs_build_hybrid(a, grouping, col_block_size, row_block_size, force_fixed_size != 0, K, kdep, &h, K > 0.0 ? &sp : nullptr, keep_order);
        if (rc == SPARTA_OK)
            rc = create_core(out, h.rows, h.cols, h.block_rows, col_block_size, h.row_part, h.nzcount, h.jab, h.mab, 0, h.block_rows, dtype, device,
                             K > 0.0 ? &sp : nullptr);
        if (rc == SPARTA_OK && K > 0.0) (*out)->ext_sparse = true;
    } catch (const std::bad_alloc&) {
        rc = fail(SPARTA_ERR_ALLOC, "sparta_vbs_create_from_csr: out of host memory");
    } catch (const std::exception& e) {
        rc = fail(SPARTA_ERR_INVALID, std::string("sparta_vbs_create_from_csr: ") + e.what());
    }
    sparta_vbs_host_free(&h);
    return rc;
}

int sparta_vbs_plan_stats(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* grouping,
                          int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size, int32_t dtype, int64_t* stats) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (!stats) return fail(SPARTA_ERR_INVALID, "sparta_vbs_plan_stats: stats is NULL");
    if (dtype != SPARTA_F32 && dtype != SPARTA_F16 && dtype != SPARTA_BF16) return fail(SPARTA_ERR_INVALID, "sparta_vbs_plan_stats: bad dtype");
    sparta::CsrView a;
    a.rows = rows; a.cols = cols; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
    double K = 24.0;
    if (const char* e = std::getenv("SPARTA_SPARSE_K")) K = atof(e);
    if (!(K > 0.0)) K = 1e-9;                                             // the sparse-row path switched off: everything is a tile
    const int64_t kdep = (dtype != SPARTA_F32 && col_block_size % 64 == 0) ? 64 : 32;
    sparta::HybridSparse sp;
    sp.esz = dtype == SPARTA_F32 ? 4.0 : 2.0;
    sp.want_union = true;
    sp.union_gran = dtype == SPARTA_F32 ? 16 : 32;
    sparta::HybridStats st;
    sparta_vbs_host h;
    std::memset(&h, 0, sizeof(h));
    const int rc = sparta::vbs_build_hybrid(a, grouping, col_block_size, row_block_size, force_fixed_size != 0, K, kdep, &h, &sp, false, &st);
    sparta_vbs_host_free(&h);
    if (rc != SPARTA_OK) return rc;
    stats[0] = st.tile_blocks; stats[1] = st.tile_area; stats[2] = (int64_t)(st.mfma_steps + 0.5); stats[3] = st.sparse_nnz; stats[4] = st.sparse_rows;
    stats[5] = st.block_rows; stats[6] = st.rows; stats[7] = (int64_t)(st.union_steps + 0.5);     // [7]: 32 x 32 steps of the column-compacted tiles (k_union.hip), not in [2]
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_plan_stats")
}

int sparta_vbs_create_from_csr(sparta_vbs_t** out, int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                               const int64_t* grouping, int64_t col_block_size, int64_t row_block_size, int32_t force_fixed_size,
                               int32_t dtype, int32_t device) {
    return create_from_csr_impl(out, rows, cols, rowptr, colidx, vals, grouping, col_block_size, row_block_size, force_fixed_size, dtype, device, false);
}

// A^T of a VBS as a device handle: with it, B * A (dense x VBS) is an ordinary product -- C^T = A^T * B^T, and a column-major
// M x rows B IS a row-major rows x M B^T (same bytes), a column-major M x cols C IS a row-major cols x M C^T.  The reference's own
// "inverted" product (cublas_blockmat_multiplyBA, src/cuda/cuda_utilities.cpp:553-721) is not a B * A; this one is.
int sparta_vbs_create_transposed(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part,
                                 const int64_t* nzcount, const int64_t* jab, const float* mab, int32_t dtype, int32_t device) {
    using sparta::fail;
    if (!out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_transposed: out is NULL");
    *out = nullptr;
    if (rows <= 0 || cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_transposed: bad dimensions or NULL index array");
    if (rows > INT32_MAX || cols > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_create_transposed: more than 2^31 - 1 rows or columns");
    try {
        // CSR of A^T: row j = column j of A, entries (reordered row i, value) ascending in i; exact zeros of the blocks are dropped
        std::vector<int64_t> rp((size_t)cols + 1, 0);
        int64_t jo = 0, mo = 0;
        for (int64_t ib = 0; ib < block_rows; ib++) {
            const int64_t h = row_part[ib + 1] - row_part[ib], nb = nzcount[ib];
            if (h < 0 || nb < 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_transposed: invalid row_part / nzcount");
            for (int64_t b = 0; b < nb; b++) {
                const int64_t c0 = jab[jo + b] * w;
                if (c0 < 0 || c0 >= cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_create_transposed: jab entry out of range");
                for (int64_t k = 0; k < w && c0 + k < cols; k++)
                    for (int64_t i = 0; i < h; i++) rp[(size_t)(c0 + k) + 1] += mab[mo + (b * w + k) * h + i] != 0.0f;
            }
            jo += nb; mo += nb * h * w;
        }
        for (int64_t j = 0; j < cols; j++) rp[(size_t)j + 1] += rp[(size_t)j];
        std::vector<int32_t> ci((size_t)rp[(size_t)cols]);
        std::vector<float> va((size_t)rp[(size_t)cols]);
        std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
        jo = 0; mo = 0;
        for (int64_t ib = 0; ib < block_rows; ib++) {
            const int64_t h = row_part[ib + 1] - row_part[ib], nb = nzcount[ib];
            for (int64_t b = 0; b < nb; b++) {
                const int64_t c0 = jab[jo + b] * w;
                for (int64_t k = 0; k < w && c0 + k < cols; k++)
                    for (int64_t i = 0; i < h; i++) {
                        const float a = mab[mo + (b * w + k) * h + i];
                        if (a != 0.0f) { const int64_t q = fill[(size_t)(c0 + k)]++; ci[(size_t)q] = (int32_t)(row_part[ib] + i); va[(size_t)q] = a; }
                    }
            }
            jo += nb; mo += nb * h * w;
        }
        // block-rows of A^T = the column blocks of A (w rows each); its column blocks are 32 reordered rows of A wide
        std::vector<int64_t> grouping((size_t)cols);
        for (int64_t j = 0; j < cols; j++) grouping[(size_t)j] = j / w;
        return create_from_csr_impl(out, cols, rows, rp.data(), ci.data(), va.data(), grouping.data(), 32, 0, 0, dtype, device, true);   // rows stay in place: they are the columns of C
    } catch (const std::bad_alloc&) {
        return fail(SPARTA_ERR_ALLOC, "sparta_vbs_create_transposed: out of host memory");
    } catch (const std::exception& e) {
        return fail(SPARTA_ERR_INVALID, std::string("sparta_vbs_create_transposed: ") + e.what());
    }
}

/* C (+)= B * A with the handle of A^T (sparta_vbs_create_transposed): B is M x rows(A), C is M x cols(A), both column-major. */
int sparta_vbs_spmm_ba(sparta_vbs_t* At, const void* B, int64_t ldb, int32_t M, void* C, int64_t ldc, int32_t accumulate, int32_t ptr_space,
                       void* stream, float* dt_ms) {
    using sparta::fail;
    if (!At) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_ba: NULL handle");
    if (M <= 0 || ldb < M || ldc < M) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_ba: need M > 0, ldb >= M, ldc >= M");
    // a column-major M x rows matrix with leading dimension ld is the row-major rows x M matrix with the same ld
    return sparta_vbs_spmm(At, B, ldb, SPARTA_ROW_MAJOR, M, C, ldc, SPARTA_ROW_MAJOR, accumulate, ptr_space, stream, SPARTA_SPMM_MFMA, dt_ms);
}

int sparta_vbs_create(sparta_vbs_t** out, int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part,
                      const int64_t* nzcount, const int64_t* jab, const float* mab, int32_t dtype, int32_t device) {
    return sparta_vbs_create_range(out, rows, cols, block_rows, w, row_part, nzcount, jab, mab, 0, block_rows, dtype, device);
}

int sparta_vbs_destroy(sparta_vbs_t* A) {
    destroy_impl(A);
    return SPARTA_OK;
}

int sparta_vbs_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_info: NULL argument");
    std::memset(info, 0, 16 * sizeof(int64_t));
    info[0] = A->rows; info[1] = A->cols; info[2] = A->block_rows; info[3] = A->w; info[4] = A->nblocks; info[5] = A->nztot;
    for (int c = 0; c < 3; c++) info[6 + c] = A->n_real_tiles[c];
    info[9] = A->n_sp_rows;                // rows handled by the sparse-row path
    info[10] = A->a_bytes; info[11] = A->exec_area;
    info[12] = A->n_steps[0] + A->n_steps[1]; info[13] = A->n_workers; info[14] = A->n_split; info[15] = A->last_path;
    return SPARTA_OK;
}

// the packed plan of an fp32 handle (vbs_plan.cpp, k_f32_packed.hip): {1 if the <= 32-row tiles run on packed steps, packed steps, slots = MFMA pairs they
// issue, steps of the one-tile plan they replace (= blocks x 32-deep slices)}
int sparta_vbs_packed_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_packed_info: NULL argument");
    info[0] = A->d_a_pack != nullptr; info[1] = A->n_psteps; info[2] = A->pack_slots; info[3] = A->dtype == SPARTA_F32 ? A->n_steps[0] : 0;
    return SPARTA_OK;
}

int sparta_vbs_flags(const sparta_vbs_t* A, int32_t* flags_out) {
    if (!A || !flags_out) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_flags: NULL argument");
    *flags_out = A->create_flags;
    return SPARTA_OK;
}

int sparta_vbs_hub_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_hub_info: NULL argument");
    info[0] = A->n_hub_steps; info[1] = A->n_hub_tiles; info[2] = A->n_hub_groups; info[3] = A->n_hub_steps > 0 ? A->hub_g : 0;
    info[4] = A->hub_area; info[5] = A->hub_union_area; info[6] = A->n_hub_steps > 0 ? A->hub_workers : 0; info[7] = A->hub_chunks; info[8] = A->hub_segments; info[9] = 0;
    return SPARTA_OK;
}

int sparta_vbs_union_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_union_info: NULL argument");
    info[0] = A->u_tiles_h[0]; info[1] = A->u_tiles_h[1]; info[2] = A->u_steps_h[0]; info[3] = A->u_steps_h[1];
    info[4] = A->u_area; info[5] = A->u_cols; info[6] = A->u_nnz; info[7] = 0;
    for (int ty = 0; ty < kUnionTypes; ty++) info[7] = std::max<int64_t>(info[7], A->u_workers[ty]);
    info[8] = A->u_rows; info[9] = A->u_tail_nnz;
    info[10] = A->u_exec_area; info[11] = A->u_steps_total > 0 ? (A->dtype == SPARTA_F32 ? 16 : 32) : 0;
    return SPARTA_OK;
}

int sparta_vbs_sparse_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_sparse_info: NULL argument");
    info[0] = A->n_sp_rows; info[1] = A->sp_nnz; info[2] = A->n_sp_short; info[3] = A->n_sp_long;
    return SPARTA_OK;
}

int sparta_vbs_colres_info(const sparta_vbs_t* A, int64_t* info) {
    if (!A || !info) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_colres_info: NULL argument");
    info[0] = A->cr_slices; info[1] = A->cr_entries; info[2] = A->cr_long; info[3] = A->cr_plane; info[4] = A->cr_lmax; info[5] = A->last_colres_nc;
    info[6] = A->cr_slices > 0 ? A->sp_nnz : 0; info[7] = A->cr_slices > 0 && A->cr_unit ? 1 : 0; info[8] = A->cr_parts; info[9] = A->cr_ranges; info[10] = A->cr_small.n_parts; info[11] = A->last_colres_small ? 1 : 0;
    return SPARTA_OK;
}

#ifdef SPARTA_TIMELINE
// developer build only: the raw timeline words (4 waves x 64 steps x 8)
int sparta_debug_timeline(sparta_vbs_t* A, long long* out) {
    if (!A || !out || !A->d_clk) return -1;
    DeviceGuard guard(A->device);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpy(out, A->d_clk + 16, (4 * 64 * 8 + 2048) * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

int sparta_debug_device_allocs(int64_t* live_count, int64_t* live_bytes) {
    if (live_count) *live_count = g_dev_live_count.load();
    if (live_bytes) *live_bytes = g_dev_live_bytes.load();
    return SPARTA_OK;
}

int sparta_vbs_clock_mhz(sparta_vbs_t* A, double* mhz_out) {
    using sparta::fail;
    if (!A || !mhz_out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_clock_mhz: NULL argument");
    DeviceGuard guard(A->device);
    for (int c = 0; c < 4; c++) mhz_out[c] = 0.0;
    if (!A->class_timing || !A->d_clk) return SPARTA_OK;
    long long h[16];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h, A->d_clk, sizeof(h), hipMemcpyDeviceToHost));
    for (int c = 0; c < 4; c++) {
        if (!A->class_ran[c]) continue;
        const long long dc = h[4 * c + 2] - h[4 * c], dr = h[4 * c + 3] - h[4 * c + 1];
        if (dr > 0 && dc > 0) mhz_out[c] = (double)dc / (double)dr * 100.0;      // s_memrealtime ticks at 100 MHz
    }
    return SPARTA_OK;
}

}  // extern "C"

namespace {

// do the <= 32-row tiles of this handle go through the C ring (CRing)?  Tiles that do not start on multiples of 32 rows AND are short (the plan kept
// contiguous worker ranges for exactly these: vbs_plan.cpp, ring_plan)
bool ring_tiles(const sparta_vbs_t* A) { return !A->tiles_row_aligned[0] && A->n_steps[0] < 6 * A->n_plan_tiles[0]; }

// cache policy of a stream launch's C stores (vbs_kernel_common.hpp): non-temporal for long tiles; SPARTA_C_NT=0|1 forces one
int32_t c_store_nt(const sparta_vbs_t* A, int ty, const float* C, int64_t ldc, bool c_row_major, bool ring = false) {
    if (const char* e = std::getenv("SPARTA_C_NT")) return atoi(e) != 0;
    if (A->n_plan_tiles[ty] <= 0) return 0;
    if (A->n_steps[ty] >= 6 * A->n_plan_tiles[ty]) return 1;                    // long tiles
    // short tiles: only when a store instruction writes whole, aligned 128-byte lines (32-row tiles starting at multiples of 32 rows of a
    // column-major C whose columns are 128-byte aligned) -- banded 200k in fixed 32-row tiles: 63 us default, 51 non-temporal; the same
    // matrix in tiles of 28 rows on average (misaligned pieces of lines): 67-71 default, 79 non-temporal
    // (`ring`: the no-barrier fp32 kernel parks tiles of arbitrary height in LDS and stores aligned blocks of 32 rows: banded 200k 51 us default, 45 non-temporal)
    return !c_row_major && (A->tiles_row_aligned[ty] || ring) && ldc % 32 == 0 && ((uintptr_t)C % 128) == 0;
}

// long runs of rows without blocks, accumulate = 0: streamed zero fill (vbs_zero_rows_kernel), one launch per run
void launch_zero_ranges(sparta_vbs_t* A, float* C, int64_t ldc, bool c_row_major, int n_cols, hipStream_t st) {
    for (const auto& zr : A->zero_ranges) {
        const int64_t n_lines = c_row_major ? zr.second : (int64_t)n_cols, line_len = c_row_major ? (int64_t)n_cols : zr.second;
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (line_len / 4 + kThreads - 1) / kThreads));
        const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_lines, 16384));
        launch_zero_rows(dim3(gx, gy), st, C, ldc, (int)c_row_major, zr.first, zr.second, n_cols);
    }
}

// step lists for a gathered B (slab index + row inside the slab): built once per slab height and kept (sparta_vbs::gathered).  A list is never rewritten:
// a graph captured at one height holds its address and must go on reading that height's steps.
int ensure_gathered_steps(sparta_vbs_t* A, int64_t shard_rows, hipStream_t st) {
    if (A->g_cur >= 0 && A->gathered[(size_t)A->g_cur].shard_rows == shard_rows) return SPARTA_OK;
    for (size_t i = 0; i < A->gathered.size(); i++)
        if (A->gathered[i].shard_rows == shard_rows) { A->g_cur = (int)i; return SPARTA_OK; }
    if (g_capturing) return capture_refusal("build the step lists of this slab height");
    sparta_vbs::GatheredSteps gs;                                // (joins the cache only when complete: a failed upload leaves no half-built set behind)
    gs.shard_rows = shard_rows;
    for (int ty = 0; ty < 2; ty++) {
        if (A->h_steps[ty].empty()) continue;
        std::vector<StepRec> g = A->h_steps[ty];
        for (StepRec& r : g) { r.pad = (int32_t)(r.b_row / shard_rows); r.b_row = (int32_t)(r.b_row % shard_rows); }
        HIP_TRY(gs.steps[ty].alloc(g.size()));
        HIP_TRY(hipMemcpyAsync(gs.steps[ty], g.data(), g.size() * sizeof(StepRec), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                       // g goes out of scope
    }
    if (!A->h_hub_steps.empty()) {
        std::vector<HubStep> g = A->h_hub_steps;
        for (HubStep& r : g) if (!(r.flags & STEP_TAIL)) { r.shard = (int32_t)(r.b_row / shard_rows); r.b_row = (int32_t)(r.b_row % shard_rows); }
        HIP_TRY(gs.hub.alloc(g.size()));
        HIP_TRY(hipMemcpyAsync(gs.hub, g.data(), g.size() * sizeof(HubStep), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    A->gathered.push_back(std::move(gs));
    A->g_cur = (int)A->gathered.size() - 1;
    return SPARTA_OK;
}

// fp32 handles whose <= 32-row tiles have a fragment image (k_f32_direct.hip) hold A twice at create time.  Once the no-barrier kernel has won the plan-time autotune on a
// handle whose blocks are ALL in that image (no 33..64-row tiles, no sparse rows), the reference-layout copy is dropped (drop_legacy_image: a_bytes = one image); a later call that reads it -- SPARTA_SPMM_EXACT, a
// row-major or gathered B, the per-class kernels -- rebuilds it on the device from the fragment image (an exact copy) and then keeps it.  SPARTA_F32_KEEP_LEGACY=1: never drop.
int ensure_legacy_image(sparta_vbs_t* A, hipStream_t st) {
    if (A->d_A || A->dtype != SPARTA_F32) return SPARTA_OK;
    if (g_capturing) return capture_refusal("rebuild the reference-layout image of A");
    const size_t bytes = (size_t)(A->nztot + 128) * sizeof(float);
    HIP_TRY(A->d_A.alloc((size_t)A->nztot + 128));
    HIP_TRY(hipMemsetAsync(A->d_A, 0, bytes, st));
    if (A->n_steps[0] > 0 && A->d_a_pack) launch_f32_legacy_from_pack(st, A->d_steps[0], A->d_pack_loc, A->n_steps[0], A->d_a_pack, A->d_A);
    else if (A->n_steps[0] > 0) launch_f32_legacy_from_frag(st, A->d_steps[0], A->n_steps[0], A->d_a_frag, A->d_A);
    HIP_TRY(hipGetLastError());
    A->a_bytes += (int64_t)bytes;
    return SPARTA_OK;
}
void drop_legacy_image(sparta_vbs_t* A) {
    static const bool keep = [] { const char* e = std::getenv("SPARTA_F32_KEEP_LEGACY"); return e && atoi(e) != 0; }();
    if (A->create_flags & SPARTA_CREATE_TRANSPOSE) return;      // sparta_vbs_spmm_t reads the reference-layout image
    if (A->retired.captured) return;                            // a captured graph may read it (a row-major or gathered B, the per-class kernels): the handle keeps both images
    if (keep || g_capturing || A->legacy_dropped || !A->d_A || !(A->d_a_frag || A->d_a_pack) || A->dtype != SPARTA_F32 || A->n_steps[1] != 0 || A->n_sp_rows != 0 || A->class_timing) return;
    A->d_A.reset();                                      // (synchronises: the autotune's launches that read it are done)
    A->a_bytes -= (int64_t)((A->nztot + 128) * sizeof(float));
    A->legacy_dropped = true;
}

// The ROW-major B of the product in flight (A->brm_ready / brm_ld; cleared when the product returns): B itself when the call's B is row-major, the caller's prepared
// copy (sparta_vbs_prepare_b), or a transposed copy made now -- ONCE per product, whoever asks first (the column-compacted tiles, then the sparse rows).  `aligned16`:
// rows must start on 16-byte boundaries (k_union.hip loads them 16 bytes per lane); the copies made here always do (row stride rounded up to 16 bytes).
int ensure_brm(sparta_vbs_t* A, const void* dB, int64_t ldb, bool b_row_major, int64_t shard_rows, int64_t shard_stride, int bk, int32_t n_cols, hipStream_t st,
               bool aligned16) {
    if (A->brm_ready) return SPARTA_OK;
    const size_t esz = bk == 0 ? 4 : 2;
    const int64_t per16 = 16 / (int64_t)esz;
    if (b_row_major && shard_rows == 0 && (!aligned16 || (ldb % per16 == 0 && ((uintptr_t)dB % 16) == 0))) { A->brm_ready = dB; A->brm_ld = ldb; return SPARTA_OK; }
    if (A->prepared_brm && !b_row_major) { A->brm_ready = A->prepared_brm; A->brm_ld = A->prepared_ld; return SPARTA_OK; }
    if (g_capturing && A->d_Brm.bytes() < (size_t)A->cols * (size_t)((n_cols + per16 - 1) / per16 * per16) * esz) return capture_refusal("allocate the row-major copy of B");
    const int64_t ld = (n_cols + per16 - 1) / per16 * per16;
    if (int rc = A->d_Brm.ensure((size_t)A->cols * (size_t)ld * esz, A->retired)) return rc;
    if (b_row_major) {                                   // (a row-major B whose rows are not 16-byte aligned: an aligned copy)
        HIP_TRY(hipMemcpy2DAsync(A->d_Brm, (size_t)ld * esz, dB, (size_t)ldb * esz, (size_t)n_cols * esz, (size_t)A->cols, hipMemcpyDeviceToDevice, st));
    } else {
        const int64_t n_wg = ((A->cols + 63) / 64) * (int64_t)((n_cols + 63) / 64);
        if (n_wg > INT32_MAX) return sparta::fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: B too large for the transpose grid");
        launch_b_to_row_major(bk != 0, (unsigned)n_wg, st, dB, ldb, shard_rows, shard_stride, A->cols, (int)n_cols, A->d_Brm, ld);
    }
    A->brm_ready = A->d_Brm; A->brm_ld = ld;
    return SPARTA_OK;
}

// the column-compacted tiles (k_union.hip): C[tile rows, :] (+)= Atile . B[list, :] on the matrix cores, B row-major.  Stores (or adds to) every row of its tiles;
// the sparse rows of those block-rows (their thinly used columns) add behind it on the same stream.
int launch_union_tiles(sparta_vbs_t* A, const void* dB, int64_t ldb, bool b_row_major, int64_t shard_rows, int64_t shard_stride, int32_t n_cols, float* dC,
                       int64_t ldc, bool c_row_major, bool accumulate, hipStream_t st) {
    if (A->u_steps_total == 0) return SPARTA_OK;
    // 32-bit byte offsets inside a tile's 64 rows x 32 columns of C
    if ((c_row_major ? 64 * ldc + 128 : 32 * ldc + 128) * 4 >= ((int64_t)1 << 31) - 65536)
        return sparta::fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: leading dimension of C too large for the column-compacted tile kernel (32-bit offsets inside a tile)");
    const int bk = A->dtype == SPARTA_F32 ? 0 : (A->dtype == SPARTA_BF16 ? 2 : 1);
    if (int rc = ensure_brm(A, dB, ldb, b_row_major, shard_rows, shard_stride, bk, n_cols, st, true)) return rc;
    UnionParams up;
    up.B = (const float*)A->brm_ready; up.ldb = A->brm_ld; up.C = dC; up.ldc = ldc;
    up.n_cols = n_cols; up.accumulate = accumulate ? 1 : 0; up.c_row_major = c_row_major ? 1 : 0;
    up.pad = [] { const char* e = std::getenv("SPARTA_UNION_PROBE"); return e ? atoi(e) : 0; }();      // developer probes (timing only, wrong products; read per call)
    for (int ty = 0; ty < kUnionTypes; ty++) {
        UnionSide& sd = up.side[ty];
        sd.rec = A->d_u_rec[ty]; sd.ids = A->d_u_ids[ty]; sd.A = A->d_u_a[ty]; sd.worker_range = A->d_u_wrange[ty]; sd.tail = (const uint2*)A->d_u_tail[ty].get();
        sd.n_workers = A->u_steps[ty] > 0 ? A->u_workers[ty] : 0;
        // C is written once and never read back: non-temporal stores where tiles are long (as the stream kernels: vbs_kernel_common.hpp); SPARTA_C_NT=0|1 forces one
        const char* e = std::getenv("SPARTA_C_NT");
        sd.c_nt = e ? (atoi(e) != 0) : (A->u_steps[ty] >= 6 * A->u_tiles[ty] ? 1 : 0);
    }
    if (bk == 0) launch_union_f32((unsigned)((n_cols + kTN - 1) / kTN), st, up);
    else launch_union_h16(bk == 2, (unsigned)((n_cols + kTN - 1) / kTN), st, up);
    HIP_TRY(hipGetLastError());
    return SPARTA_OK;
}

int launch_sparse_rows(sparta_vbs_t* A, const void* dB, int64_t ldb, bool b_row_major, int64_t shard_rows, int64_t shard_stride, int bk,
                       int32_t n_cols, float* dC, int64_t ldc, bool c_row_major, bool accumulate, hipStream_t st) {
    const size_t esz = bk == 0 ? 4 : 2;
    A->last_colres_nc = 0;
    // Small A, the reference's own layouts (column-major B and C): the resident-column product -- NC columns of B in LDS, A streamed past them from L2, one launch
    // (k_colres.hip).  No transpose of B, no partial rows, B and C cross HBM once.
    if (bk == 0 && A->cr_slices > 0 && !b_row_major && !c_row_major && shard_rows == 0) {
        const int nc = colres_columns(A, n_cols);
        if (nc > 0) {
            int nc_used = nc;
            bool used_small = false;
            ColresParams cp;
            cp.col4 = (const uint2*)A->d_cr_col.get(); cp.val4 = (const float4*)A->d_cr_val.get(); cp.parts = A->d_cr_parts; cp.meta = A->d_cr_meta;
            cp.dest = A->d_cr_dest; cp.longs = (const ColresLong*)A->d_cr_longs; cp.mode = (const uint8_t*)A->d_cr_mode;
            cp.B = (const float*)dB; cp.ldb = ldb; cp.C = dC; cp.ldc = ldc;
            for (int r = 0; r <= kColresMaxRanges; r++) cp.krange[r] = A->cr_krange[r];
            cp.n_parts = A->cr_parts; cp.n_ranges = A->cr_ranges; cp.N = n_cols; cp.accumulate = accumulate ? 1 : 0;
            cp.vec_out = ldc % 4 == 0 && ((uintptr_t)dC % 16) == 0 ? 1 : 0;
            cp.vec_in = ldb % 4 == 0 && ((uintptr_t)dB % 16) == 0 ? 1 : 0;
            cp.probe = [] { const char* e = std::getenv("SPARTA_COLRES_PROBE"); return e ? atoi(e) : 0; }();        // (read per call: developer A/B)
            size_t lds_bytes = (size_t)A->cr_plane * (size_t)nc * sizeof(float);
            // few column sets: the four-part image, the fewest columns per workgroup that keep the product one round of workgroups (read per call: SPARTA_COLRES_SMALL=0 keeps the whole image)
            if (A->cr_small.slices > 0) {
                const char* es = std::getenv("SPARTA_COLRES_SMALL");
                const char* en = std::getenv("SPARTA_COLRES_NC");
                const int fit = (int)std::min<int64_t>(std::min<int64_t>(4, kColresCells / A->cr_plane), n_cols);
                int ncs = 0;
                for (int c = 1; c <= fit && ncs == 0; c++) if ((int64_t)((n_cols + c - 1) / c) * A->cr_small.n_parts <= 256 && A->cr_small.slices <= colres_max_slices(c)) ncs = c;
                if (ncs > 0 && !en && !(es && atoi(es) == 0)) {
                    nc_used = ncs; used_small = true;
                    cp.col4 = (const uint2*)A->cr_small.col.get(); cp.val4 = (const float4*)A->cr_small.val.get(); cp.parts = A->cr_small.parts; cp.meta = A->cr_small.meta;
                    cp.dest = A->cr_small.dest; cp.longs = (const ColresLong*)A->cr_small.longs;
                    cp.n_parts = A->cr_small.n_parts;
                    lds_bytes = (size_t)A->cr_plane * (size_t)ncs * sizeof(float);
                }
            }
            {
                static const int n_cus = [] { hipDeviceProp_t pr; return hipGetDeviceProperties(&pr, 0) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }();
                cp.n_cus = n_cus;
                // start the CUs in three groups, a quarter of a workgroup's time apart (its stream of A: LDS-bound, ~7 / 7 / 14 / 13 cycles per step of 64 slots with 1..4 columns;
                // its columns of B and C at HBM speed).  Measured at N = 8192 (profiles/r4/lab_colres_stagger2.txt): bcsstk18 0.262 -> 0.234 ms, wiki-Vote 0.217 -> 0.189,
                // ca-HepPh 0.326 -> 0.294; two groups or four, or offsets of half a workgroup's time: less or nothing.  SPARTA_COLRES_STAGGER_US / SPARTA_COLRES_GROUPS:
                // developer A/B, read per call; 0 = everybody at once
                static const double step_cycles[5] = {0.0, 7.0, 7.0, 14.0, 13.0};
                const double t_wg = (double)A->cr_entries / 64.0 * step_cycles[nc] / 2.4e9 + (double)(A->rows + A->cols) * nc * 4.0 / (6.0e12 / n_cus) + 3.0e-6;
                const char* e = std::getenv("SPARTA_COLRES_STAGGER_US");
                const char* eg = std::getenv("SPARTA_COLRES_GROUPS");
                cp.share = eg ? std::max(1, atoi(eg)) : 3;
                const double stagger = e ? atof(e) * 1e-6 : t_wg / 4.0;
                cp.stagger_ticks = cp.share > 1 && (int64_t)((n_cols + nc_used - 1) / nc_used) * cp.n_parts > 2 * (int64_t)n_cus ? (int32_t)std::min(stagger * 1e8, 1.0e5) : 0;
            }
            if (int hrc = launch_colres(nc_used, cp, lds_bytes, st)) return sparta::fail(SPARTA_ERR_HIP, "sparta_vbs_spmm: the resident-column kernel could not be launched (hipError_t " + std::to_string(hrc) + ")");
            HIP_TRY(hipGetLastError());
            A->last_colres_nc = nc_used; A->last_colres_small = used_small;
            return SPARTA_OK;
        }
    }
    SparseParams q;
    q.rowptr = A->d_sp_rowptr; q.col = A->d_sp_col; q.val = A->d_sp_val; q.crow = A->d_sp_crow;
    q.list = nullptr; q.n_list = 0;
    q.N = n_cols; q.accumulate = accumulate;
    q.b_col_stride = 0; q.shard_rows = 0; q.shard_stride = 0;
    // A column-major B read in place costs one 64-byte line per ELEMENT (16 x the bytes of a row-major row); transposing costs
    // 2 x |B| once.  In place wins while  nnz * 16 < 2 * cols.
    // SPARTA_SP_INPLACE = 0 | 1 forces the choice (developer A/B)
    static const int inplace_env = [] { const char* e = std::getenv("SPARTA_SP_INPLACE"); return e ? atoi(e) : -1; }();
    // (a row-major copy the column-compacted tiles of this product already made is used, whatever the count)
    const bool in_place = !(b_row_major && shard_rows == 0) && !A->brm_ready && (inplace_env >= 0 ? inplace_env != 0 : A->sp_nnz * 8 < A->cols);
    if (b_row_major && shard_rows == 0) { q.B = dB; q.ldb = ldb; }
    else if (in_place) { q.B = dB; q.ldb = 0; q.b_col_stride = ldb; q.shard_rows = shard_rows; q.shard_stride = shard_stride; }
    else {                                               // sparta_vbs_prepare_b: transposed once; else now, once per product (ensure_brm)
        if (int rc = ensure_brm(A, dB, ldb, b_row_major, shard_rows, shard_stride, bk, n_cols, st, false)) return rc;
        q.B = A->brm_ready; q.ldb = A->brm_ld;
    }
    // round 4: (column, value) pairs through scalar loads and the row of B as an SGPR base (k_sparse.hip: sparse_row_partial_s) -- rows of B shorter than 4 GB (the
    // row offset is a 32 x 32 -> 64 bit scalar multiply); SPARTA_SP_SCALAR=0: the round-3 gather (developer A/B; read per call)
    {
        const char* e = std::getenv("SPARTA_SP_SCALAR");
        q.scalar_gather = (e ? atoi(e) != 0 : true) && q.b_col_stride == 0 && q.ldb * (int64_t)esz < ((int64_t)1 << 32) ? 1 : 0;
    }
    // the kernels write C themselves: rows of a row-major C, or 16-row pieces of the columns of the reference's column-major C
    q.out = dC; q.ldo = ldc; q.out_is_c = c_row_major ? 1 : 2;
    if (A->n_sp_long > 0)
        if (int rc = A->d_sp_part.ensure((size_t)A->n_sp_segs * (size_t)n_cols * sizeof(float), A->retired)) return rc;
    // widest vector the shapes allow: every row start VEC-element aligned, N a multiple of 64 * VEC (no ragged chunk)
    auto aligned = [&](int v) {
        const bool out_ok = q.out_is_c == 2 || (q.ldo % v == 0 && ((uintptr_t)q.out % (4 * v)) == 0);
        return n_cols % (64 * v) == 0 && q.ldb % v == 0 && out_ok && ((uintptr_t)q.B % (esz * v)) == 0;
    };
    // How many columns of C a wave takes = how many bytes of a row of B one gather instruction reads.  A workgroup column (grid y) is walked
    // to the end before the next starts, so the bytes per row set how many rows of B an XCD's 4 MiB L2 holds while the rows that reference
    // them go by: on power-law inputs the hub rows of B stay resident with narrow chunks and are pushed out by wide ones.  Measured
    // (R-MAT, 10 edges per row, fp32 N = 256 | bf16 N = 512; ms per product at 1024 / 512 / 256 bytes per row): 2^20 rows (|B| = 1 GiB)
    // 4.33 / 3.92 / 3.77 | - / 4.54 / 4.27; 2^18 rows (256 MiB) 0.93 / 0.87 / 0.89 | - / 1.02 / 1.03; 2^16 rows and below: widest wins
    // by 3-10 %.  2-byte loads (one bf16 per lane) are slow whatever the size (6.6 ms) and never chosen.  SPARTA_SP_VEC caps the width.
    static const int vec_cap = [] { const char* e = std::getenv("SPARTA_SP_VEC"); return e ? atoi(e) : 4; }();
    const double b_bytes = (double)A->cols * (double)n_cols * (double)esz;
    const int row_bytes_env = [] { const char* e = std::getenv("SPARTA_SP_ROW_BYTES"); return e ? atoi(e) : 0; }();      // (read per call: developer A/B)
    // (what matters is the SLICE of B one column chunk touches, cols x row_bytes: while that fits the Infinity Cache the widest chunk wins -- the reference's real
    // matrices at its operand width N = 8192, 8-58 k columns, |B| = 0.3-1.9 GB: 1.14 -> 0.83 ms (bcsstk18), 3.37 -> 2.81 (social_location) with 1024 instead of 256)
    const bool slice_fits = (double)A->cols * 1024.0 <= 96e6;
    const int row_bytes = row_bytes_env > 0 ? row_bytes_env : (slice_fits ? 1024 : (b_bytes > 384e6 ? 256 : (b_bytes > 96e6 ? 512 : 1024)));
    const int vec_want = std::max(esz == 2 ? 2 : 1, std::min(vec_cap, (int)(row_bytes / (64 * (int)esz))));
    const int vec = in_place ? 1 : (vec_want >= 4 && aligned(4) ? 4 : (vec_want >= 2 && aligned(2) ? 2 : 1));
    const unsigned gy = (unsigned)((n_cols + 64 * vec - 1) / (64 * vec));
    launch_sparse_kernels(vec, bk, q, gy, st, A->d_sp_list, A->n_sp_short, (const SpSegRec*)A->d_sp_segs, A->n_sp_segs, (const SpLongRec*)A->d_sp_long,
                          A->n_sp_long, (float*)A->d_sp_part, A->d_sp_stream_begin, A->sp_max_stream);
    HIP_TRY(hipGetLastError());
    return SPARTA_OK;
}

// 16-bit handles (SPARTA_F16 / SPARTA_BF16): A and B in the 16-bit type, fp32 accumulation, fp32 C.  Device pointers: B is a
// 16-bit column-major matrix (ldb in elements, even).  Host pointers keep the reference's contract (fp32 B in, fp32 C out):
// B is converted on the device (round to nearest even).  This is the product over whole 128-column slabs; spmm16_impl (below) cuts a
// call with any other n_cols into whole slabs + one padded tail slab.
int spmm16_core(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int64_t shard_rows, int64_t shard_stride, int32_t n_cols, void* C,
                int64_t ldc, int32_t c_layout, int32_t accumulate, int32_t ptr_space, hipStream_t st, int32_t algo, float* dt_ms) {
    using sparta::fail;
    if (algo != SPARTA_SPMM_MFMA) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: SPARTA_SPMM_EXACT needs an fp32 handle");
    if (shard_rows != 0 && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: device pointers only");
    if (b_layout != SPARTA_COL_MAJOR) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: 16-bit handles need a column-major B (k contiguous)");
    if (n_cols % kTN != 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: internal: the 16-bit core takes whole 128-column slabs");
    const bool bf16 = A->dtype == SPARTA_BF16;
    const size_t c_elems = (size_t)ldc * (size_t)(c_layout == SPARTA_COL_MAJOR ? n_cols : A->rows);
    const uint16_t* dB = (const uint16_t*)B;
    float* dC = (float*)C;
    int64_t ldb16 = ldb;
    if (ptr_space == SPARTA_PTR_HOST) {
        const size_t b_elems = (size_t)ldb * (size_t)n_cols;
        ldb16 = (A->cols + 7) / 8 * 8;
        if (int rc = A->d_B.ensure(b_elems * sizeof(float), A->retired)) return rc;
        if (int rc = A->d_B16.ensure((size_t)ldb16 * n_cols * sizeof(uint16_t), A->retired)) return rc;
        if (int rc = A->d_C.ensure(c_elems * sizeof(float), A->retired)) return rc;
        HIP_TRY(hipMemcpyAsync(A->d_B, B, b_elems * sizeof(float), hipMemcpyHostToDevice, st));
        if (accumulate) HIP_TRY(hipMemcpyAsync(A->d_C, C, c_elems * sizeof(float), hipMemcpyHostToDevice, st));
        else if (c_elems > 0) HIP_TRY(hipMemsetAsync(A->d_C, 0, c_elems * sizeof(float), st));
        launch_convert_h16(bf16, st, (const float*)A->d_B, ldb, A->cols, (int64_t)n_cols, (uint16_t*)A->d_B16, ldb16);
        dB = (const uint16_t*)A->d_B16;
        dC = (float*)A->d_C;
    } else if (ldb % 2 != 0) {
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: 16-bit B needs an even leading dimension (16-byte loads start on 4-byte boundaries)");
    }
    // 32-bit byte offsets: the no-barrier kernel keeps them inside ONE WAVE's 32 columns (31 x ld x element size < 2^31: ldb < 34 M, ldc < 17 M elements;
    // its 64-column waves span 64 columns of B: ldb < 16 M);
    // the LDS-staged kernel (SPARTA_H16_PATH=lds) inside the 128-column slab (ldb < 8.3 M, ldc < 4.1 M)
    {
        const bool direct = h16_uses_direct_kernel(A->kp16, false) || A->wide16;
        const int64_t span_b = A->wide16 ? 64 : direct ? 32 : 128, span_c = direct ? 32 : 128;       // columns a wave's 32-bit offsets span (64-column waves: B only)
        if (ldb16 * span_b * 2 >= ((int64_t)1 << 31) - 65536 || (c_layout == SPARTA_ROW_MAJOR ? ldc * 32 : ldc * span_c) * 4 >= ((int64_t)1 << 31) - 65536)
            return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: leading dimension too large for the 16-bit stream kernels (ldb < 34 M -- 16 M for one-tile plans of "
                                                "32-wide blocks -- and ldc < 17 M elements; 8.3 M / 4.1 M with SPARTA_H16_PATH=lds)");
    }
    if (dt_ms) HIP_TRY(hipEventRecord(A->ev0, st));
    const int n_nt = n_cols / kTN;
    const bool prof = A->class_timing;
    for (int c = 0; c < 4; c++) A->class_ran[c] = false;
    const size_t slab = (size_t)A->n_slots * SK_SLOT_FLOATS;
    if (A->n_split > 0)
        if (int rc = A->d_ws.ensure(slab * n_nt * sizeof(float), A->retired)) return rc;
    StreamParams sp;
    sp.A = A->d_A; sp.B = (const float*)dB; sp.C = dC; sp.ws = (float*)A->d_ws;
    sp.ldb = ldb16; sp.ldc = ldc; sp.cols = A->cols; sp.shard_rows = shard_rows; sp.shard_stride = shard_stride;
    if (shard_rows > 0)
        if (int rc = ensure_gathered_steps(A, shard_rows, st)) return rc;
    sp.ws_slab_stride = (int64_t)slab; sp.accumulate = accumulate != 0; sp.c_row_major = c_layout == SPARTA_ROW_MAJOR;
    sp.N = n_cols; sp.w = (int32_t)A->w; sp.B_tail = nullptr; sp.clk = nullptr; sp.stagger = 0;
    if (A->n_steps[0] + A->n_steps[1] + A->n_hub_steps > 0) {
        if (prof) HIP_TRY(hipEventRecord(A->cev[0][0], st));
        if (A->has_tail && shard_rows == 0) {
            if (int rc = A->d_btail.ensure((size_t)A->w * n_cols * sizeof(uint16_t), A->retired)) return rc;
            const int64_t row0 = ((A->cols - 1) / A->w) * A->w;
            launch_tail_copy_h16(st, dB, ldb16, row0, A->cols, (int)A->w, (int)n_cols, (uint16_t*)A->d_btail);
            sp.B_tail = (const float*)A->d_btail;
        }
        const dim3 grid((unsigned)A->n_workers, (unsigned)n_nt);
        const int probe_ty = A->n_steps[1] >= A->n_steps[0] ? 1 : 0;
        // live forward (sparta_vbs_set_live_forward): with a live set installed and the switch on, the stream image that has compacted records is walked by
        // the live kernels (k_h16_live.hip) on them; read here, when the product is called or captured.  Not for a gathered B.
        const bool fwd_live = A->live_on && A->live_fwd && A->live_fwd_built && A->live_fwd_ty >= 0 && shard_rows == 0;
        // the fp8 weight image (sparta_vbs_set_forward_a8): with the switch on and a valid image, the stream image that has one is multiplied by the a8 kernels
        // (k_h16_a8.hip) from the codes, on the handle's private records.  Not for a gathered B; never together with live forward (the switches exclude each other).
        const bool fwd_a8 = A->a8_on && A->a8_valid && A->a8_built && A->a8_ty >= 0 && shard_rows == 0;
        for (int ty = 1; ty >= 0; ty--) {
            if (A->n_steps[ty] == 0) continue;
            sp.steps = shard_rows > 0 ? A->gathered[(size_t)A->g_cur].steps[ty] : A->d_steps[ty]; sp.worker_range = A->d_wrange[ty]; sp.c_nt = c_store_nt(A, ty, sp.C, sp.ldc, sp.c_row_major != 0);
            sp.clk = (prof && ty == probe_ty) ? A->d_clk : nullptr;
            const bool gth = shard_rows > 0;
            // tiles of <= 32 rows of arbitrary height + column-major C: finished tiles wait in the LDS ring for whole aligned blocks (CRing)
            const int cst = [] { const char* e = std::getenv("SPARTA_CSTAGE"); return e ? atoi(e) : -1; }();
            const bool c_stage = ty == 0 && !gth && c_layout == SPARTA_COL_MAJOR && (cst >= 0 ? cst != 0 : ring_tiles(A)) && h16_uses_direct_kernel(A->kp16, false);
            if (c_stage) sp.c_nt = c_store_nt(A, ty, sp.C, sp.ldc, false, true);
            // (the a8 kernels exist where the live ones do, in their 128-column forms: a call that takes them takes neither the 256-column slab nor the four accumulators)
            const bool a8_form = fwd_a8 && ty == A->a8_ty && h16_live_form_available(A->kp16, ty != 0, c_stage && !(ty == 0 && A->wide16), ty == 0 && A->wide16);
            // 256-column slabs for the one-tile plan of 32-wide blocks (A read once per 256 columns; flagship matrix, N = 256: 42.2 -> 35.7 us, N = 512: 88.0 -> 77.0):
            // N % 256 == 0, no split tile, not through the ring, the plain plan (on the plan with two sub-worker ranges per workgroup a workgroup walks its tiles in
            // two ascending passes and the gain is gone: 41.1 us; allowed there with SPARTA_H16_SLAB256=2).  SPARTA_H16_SLAB256=0: off.
            const bool slab256 = ty == 0 && A->kp16 == 32 && !gth && !c_stage && A->n_split == 0 && n_cols % 256 == 0 && h16_uses_direct_kernel(32, false) && ldb16 * 64 * 2 < ((int64_t)1 << 31) - 65536 &&
                                 [&] { const char* e = std::getenv("SPARTA_H16_SLAB256"); const int m = e ? atoi(e) : 1; return m == 2 || (m == 1 && !A->wide16); }() &&
                                 !(fwd_live && ty == A->live_fwd_ty && A->wide16) &&    // (live ranges of two sub-workers are not adjacent: the non-slab kernel there)
                                 !a8_form;
            // 64-row tiles of 64-wide blocks (the dense hub of a power-law matrix under the fixed 64 x 64 grid), N % 256 == 0: four accumulators per wave over
            // 256-column slabs -- A read once per 256 columns, every B fragment used twice (k_h16.hip, QUAD); split tiles allowed.  SPARTA_H16_QUAD=0: off.
            const bool quad = ty == 1 && n_cols % 256 == 0 && h16_uses_direct_kernel(A->kp16, true) && ldb16 * 64 * 2 < ((int64_t)1 << 31) - 65536 &&
                              [] { const char* e = std::getenv("SPARTA_H16_QUAD"); return !e || atoi(e) != 0; }() && !a8_form;
            const bool wide = ty == 0 && A->wide16;
            const bool live_form = fwd_live && ty == A->live_fwd_ty && (quad || slab256 || h16_live_form_available(A->kp16, ty != 0, c_stage && !wide, wide));
            // the fp8 image with a live-block set (sparta_vbs_set_a8_live): the a8 launch on the compacted records and live ranges of live forward, whose last
            // words hold the exponents (vbs_q8lv_scales_kernel, k_h16_a8_live.hip).  The same instantiations as the a8 form, so the same exclusions.
            const bool a8_live_form = a8_form && A->a8_live && A->live_on && A->live_fwd_built && A->live_fwd_ty == ty;
            A->fwd_last_form[ty] = a8_live_form ? 4 : a8_form ? 3 : live_form ? 2 : 1;
            if (a8_live_form) {
                sp.A = reinterpret_cast<const float*>(A->d_a8.get()); sp.steps = A->d_fwd_steps; sp.worker_range = A->d_fwd_wrange; sp.sub_ranges = 0;
                launch_h16_a8_live_stream(A->kp16, ty != 0, bf16, c_stage, wide, grid, st, sp);
                sp.A = A->d_A;
            } else if (a8_form) {
                sp.A = reinterpret_cast<const float*>(A->d_a8.get()); sp.steps = A->d_a8_steps; sp.sub_ranges = 0;
                launch_h16_a8_stream(A->kp16, ty != 0, bf16, c_stage, wide, grid, st, sp);
                sp.A = A->d_A;
            } else if (live_form) {
                sp.steps = A->d_fwd_steps; sp.worker_range = A->d_fwd_wrange; sp.sub_ranges = 0;
                if (quad) launch_h16_live_quad(A->kp16, bf16, dim3((unsigned)A->n_workers, (unsigned)(n_cols / 256)), st, sp);
                else if (slab256) launch_h16_live_slab256(bf16, dim3((unsigned)A->n_workers, (unsigned)(n_cols / 256)), st, sp);
                else launch_h16_live_stream(A->kp16, ty != 0, bf16, c_stage, wide, grid, st, sp);
            } else if (quad) {
                sp.sub_ranges = 0;
                launch_h16_quad(A->kp16, bf16, gth, dim3((unsigned)A->n_workers, (unsigned)(n_cols / 256)), st, sp);
            } else if (slab256) {
                sp.sub_ranges = A->wide16 ? 1 : 0;
                launch_h16_slab256(bf16, dim3((unsigned)A->n_workers, (unsigned)(n_cols / 256)), st, sp);
                sp.sub_ranges = 0;
            } else
                launch_h16_stream(A->kp16, ty != 0, bf16, gth, c_stage, ty == 0 && A->wide16, grid, st, sp);
        }
        // the hub plan: group tiles of 2 / 4 long 64-row tiles through the GEMM-shaped kernel (k_hub16.hip), 256-column slabs (the last one may be a half slab)
        if (A->n_hub_steps > 0) {
            HubParams hp;
            hp.steps = shard_rows > 0 ? A->gathered[(size_t)A->g_cur].hub : A->d_hub_steps; hp.worker_range = A->d_hub_wrange; hp.tiles = A->d_hub_tiles; hp.A = A->d_hub_A;
            hp.B = dB; hp.B_tail = (const uint16_t*)sp.B_tail; hp.C = dC; hp.ws = (float*)A->d_ws;
            hp.ldb = ldb16; hp.ldc = ldc; hp.shard_stride = shard_stride; hp.ws_slab_stride = (int64_t)slab;
            hp.accumulate = accumulate != 0; hp.c_row_major = c_layout == SPARTA_ROW_MAJOR; hp.c_nt = 1; hp.w = (int32_t)A->w;
            hp.n_slabs = (n_cols + 255) / 256; hp.n_workers = A->hub_workers; hp.n_cols = n_cols; hp.pad0 = 0;
            static const int hub_variant_env = [] { const char* e = std::getenv("SPARTA_HUB_VARIANT"); return e ? atoi(e) : -1; }();
            int variant = A->hub_g == 4 ? 10 : 0;                        // KP 64: G = 4 two stages (eight waves), G = 2 three stages
            if (hub_variant_env >= 0 && hub_variant_kp(hub_variant_env) == 64 && hub_variant_g(hub_variant_env) == A->hub_g) variant = hub_variant_env;
            // a wave's panel loads span 64 (G = 2) or 32 (G = 4) columns of B in 32-bit buffer offsets: the leading dimension must keep them inside the descriptor's 2 GB
            if (ldb16 * (int64_t)(hub_variant_g(variant) == 2 ? 64 : 32) * 2 >= ((int64_t)1 << 31) - 65536)
                return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: leading dimension of B too large for the 16-bit hub kernel (32-bit panel offsets)");
            launch_h16_hub(variant, bf16, shard_rows > 0, st, hp);
        }
        if (prof) { HIP_TRY(hipEventRecord(A->cev[0][1], st)); A->class_ran[0] = true; }
    }
    const bool fix_launch = A->n_fix > 0 && !(accumulate && A->n_split == 0);   // C += 0 for the block-rows without blocks: nothing to launch
    const bool zero_launch = !A->zero_ranges.empty() && !accumulate;
    if (fix_launch || zero_launch) {
        if (prof) HIP_TRY(hipEventRecord(A->cev[1][0], st));
        if (fix_launch && A->n_big_fix > 0)
            launch_fixup_group(dim3((unsigned)A->n_big_fix, (unsigned)n_nt, (unsigned)((A->max_tile_slots + kFixGroup - 1) / kFixGroup)), st, A->d_fix,
                               A->d_big_fix, A->d_fix_slots, (float*)A->d_ws, (int64_t)slab);
        if (fix_launch)
            launch_fixup(dim3((unsigned)A->n_fix, (unsigned)n_nt), st, A->d_fix, A->d_fix_slots, (const float*)A->d_ws, (int64_t)slab, dC, ldc,
                         (int)(c_layout == SPARTA_ROW_MAJOR), (int)(accumulate != 0));
        if (zero_launch) launch_zero_ranges(A, dC, ldc, c_layout == SPARTA_ROW_MAJOR, n_cols, st);
        if (prof) { HIP_TRY(hipEventRecord(A->cev[1][1], st)); A->class_ran[1] = true; }
    }
    // (a 16-bit product runs this core once per piece of B -- the whole slabs, then the padded tail slab: each piece has its own row-major copy, made by whoever needs it first)
    A->brm_ready = nullptr; A->brm_ld = 0;
    struct BrmPiece { sparta_vbs_t* a; ~BrmPiece() { a->brm_ready = nullptr; a->brm_ld = 0; } } brm_piece{A};
    if (A->u_steps_total > 0) {   // column-compacted tiles (k_union.hip, 16-bit form): they store every row of their block-rows; those block-rows' sparse rows add, below
        const bool rec = prof && !A->class_ran[2];
        if (rec) HIP_TRY(hipEventRecord(A->cev[2][0], st));
        if (int rc = launch_union_tiles(A, dB, ldb16, false, shard_rows, shard_stride, n_cols, dC, ldc, c_layout == SPARTA_ROW_MAJOR, accumulate != 0, st)) return rc;
        if (rec) { HIP_TRY(hipEventRecord(A->cev[2][1], st)); A->class_ran[2] = true; }
    }
    if (A->n_sp_rows > 0) {                  // nearly empty block-rows: sparse rows over a row-major 16-bit copy of B
        if (prof) HIP_TRY(hipEventRecord(A->cev[3][0], st));
        if (int rc = launch_sparse_rows(A, dB, ldb16, false, shard_rows, shard_stride, bf16 ? 2 : 1, n_cols, dC, ldc, c_layout == SPARTA_ROW_MAJOR, accumulate != 0, st)) return rc;
        if (prof) { HIP_TRY(hipEventRecord(A->cev[3][1], st)); A->class_ran[3] = true; }
    }
    A->last_path = 1;
    HIP_TRY(hipGetLastError());
    if (dt_ms) {
        HIP_TRY(hipEventRecord(A->ev1, st));
        HIP_TRY(hipEventSynchronize(A->ev1));
        HIP_TRY(hipEventElapsedTime(dt_ms, A->ev0, A->ev1));
    }
    if (ptr_space == SPARTA_PTR_HOST) {
        HIP_TRY(hipMemcpyAsync(C, A->d_C, c_elems * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SPARTA_OK;
}

// Any n_cols on a 16-bit handle (the reference's `-c` is arbitrary, include/input.h:15-42): the whole 128-column slabs go through the
// kernels as they are; the last n_cols % 128 columns of B are copied (they are contiguous in a column-major B: one copy, per slab of a
// gathered B one row of a 2-D copy) into a zero-padded 128-column slab, multiplied by the same kernels into a scratch slab of C, and their
// n_cols % 128 columns merged into the caller's C (either layout, accumulate or not).  Costs scratch of 128 columns of B and of C, only
// on calls that have such a tail.
int spmm16_impl(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int64_t shard_rows, int64_t shard_stride, int32_t n_cols, void* C,
                int64_t ldc, int32_t c_layout, int32_t accumulate, int32_t ptr_space, hipStream_t st, int32_t algo, float* dt_ms) {
    using sparta::fail;
    if (n_cols % kTN == 0) return spmm16_core(A, B, ldb, b_layout, shard_rows, shard_stride, n_cols, C, ldc, c_layout, accumulate, ptr_space, st, algo, dt_ms);
    if (algo != SPARTA_SPMM_MFMA) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: SPARTA_SPMM_EXACT needs an fp32 handle");
    if (shard_rows != 0 && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: device pointers only");
    if (b_layout != SPARTA_COL_MAJOR) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: 16-bit handles need a column-major B (k contiguous)");
    const bool bf16 = A->dtype == SPARTA_BF16;
    const int32_t n_main = n_cols / kTN * kTN, n_t = n_cols - n_main;
    const size_t c_elems = (size_t)ldc * (size_t)(c_layout == SPARTA_COL_MAJOR ? n_cols : A->rows);
    const uint16_t* dB = (const uint16_t*)B;
    float* dC = (float*)C;
    int64_t ldb16 = ldb;
    if (ptr_space == SPARTA_PTR_HOST) {                    // stage here (the core's own staging assumes whole slabs)
        const size_t b_elems = (size_t)ldb * (size_t)n_cols;
        ldb16 = (A->cols + 7) / 8 * 8;
        if (int rc = A->d_B.ensure(b_elems * sizeof(float), A->retired)) return rc;
        if (int rc = A->d_B16.ensure((size_t)ldb16 * n_cols * sizeof(uint16_t), A->retired)) return rc;
        if (int rc = A->d_C.ensure(c_elems * sizeof(float), A->retired)) return rc;
        HIP_TRY(hipMemcpyAsync(A->d_B, B, b_elems * sizeof(float), hipMemcpyHostToDevice, st));
        if (accumulate) HIP_TRY(hipMemcpyAsync(A->d_C, C, c_elems * sizeof(float), hipMemcpyHostToDevice, st));
        else if (c_elems > 0) HIP_TRY(hipMemsetAsync(A->d_C, 0, c_elems * sizeof(float), st));
        launch_convert_h16(bf16, st, (const float*)A->d_B, ldb, A->cols, (int64_t)n_cols, (uint16_t*)A->d_B16, ldb16);
        dB = (const uint16_t*)A->d_B16;
        dC = (float*)A->d_C;
    } else if (ldb % 2 != 0 && shard_rows == 0) {
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: 16-bit B needs an even leading dimension (16-byte loads start on 4-byte boundaries)");
    }
    if (dt_ms) HIP_TRY(hipEventRecord(A->tev0, st));
    // (1) the whole slabs
    if (n_main > 0)
        if (int rc = spmm16_core(A, dB, ldb16, b_layout, shard_rows, shard_stride, n_main, dC, ldc, c_layout, accumulate, SPARTA_PTR_DEVICE, st, algo, nullptr)) return rc;
    // (2) the tail slab: n_t columns of B + zero columns
    const int64_t n_shards = shard_rows > 0 ? A->cols / shard_rows : 1;
    const int64_t ld_t = shard_rows > 0 ? shard_rows : ldb16;                     // rows of a column of the tail slab of B
    const size_t bt_elems = (size_t)ld_t * kTN * (size_t)n_shards;
    if (int rc = A->d_Bt.ensure(bt_elems * sizeof(uint16_t), A->retired)) return rc;
    if (int rc = A->d_Ct.ensure((size_t)A->rows * kTN * sizeof(float), A->retired)) return rc;
    HIP_TRY(hipMemsetAsync(A->d_Bt, 0, bt_elems * sizeof(uint16_t), st));
    if (shard_rows > 0 && ldb16 == shard_rows)
        HIP_TRY(hipMemcpy2DAsync(A->d_Bt, (size_t)shard_rows * kTN * sizeof(uint16_t), dB + (size_t)n_main * shard_rows, (size_t)shard_stride * sizeof(uint16_t),
                                 (size_t)n_t * shard_rows * sizeof(uint16_t), (size_t)n_shards, hipMemcpyDeviceToDevice, st));
    else if (shard_rows > 0)                                  // columns of a slab ldb16 > shard_rows apart (sparta_vbs_spmm_gathered_ld): one 2-D copy per slab
        for (int64_t sh = 0; sh < n_shards; sh++)
            HIP_TRY(hipMemcpy2DAsync((uint16_t*)A->d_Bt + (size_t)sh * shard_rows * kTN, (size_t)shard_rows * sizeof(uint16_t), dB + (size_t)sh * shard_stride + (size_t)n_main * ldb16,
                                     (size_t)ldb16 * sizeof(uint16_t), (size_t)shard_rows * sizeof(uint16_t), (size_t)n_t, hipMemcpyDeviceToDevice, st));
    else
        HIP_TRY(hipMemcpyAsync(A->d_Bt, dB + (size_t)n_main * ldb16, ((size_t)(n_t - 1) * ldb16 + (size_t)A->cols) * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));   // (not past the last column's rows: a caller may have allocated ldb * (n_cols - 1) + cols)
    {
        // the tail slab is a B of its own (zero-padded copy of the last columns): a prepared row-major copy of the caller's B does not describe it
        struct Unprepare { sparta_vbs_t* a; const void* keep; ~Unprepare() { a->prepared_brm = keep; } } unprep{A, A->prepared_brm};
        A->prepared_brm = nullptr;
        if (int rc = spmm16_core(A, A->d_Bt, ld_t, b_layout, shard_rows, shard_rows > 0 ? shard_rows * kTN : 0, kTN, A->d_Ct, A->rows, SPARTA_COL_MAJOR, 0,
                                 SPARTA_PTR_DEVICE, st, algo, nullptr)) return rc;
    }
    launch_col_tail_merge(st, (const float*)A->d_Ct, A->rows, dC, ldc, (int)(c_layout == SPARTA_ROW_MAJOR), n_main, n_t, (int)(accumulate != 0));
    HIP_TRY(hipGetLastError());
    if (dt_ms) {
        HIP_TRY(hipEventRecord(A->tev1, st));
        HIP_TRY(hipEventSynchronize(A->tev1));
        HIP_TRY(hipEventElapsedTime(dt_ms, A->tev0, A->tev1));
    }
    if (ptr_space == SPARTA_PTR_HOST) {
        HIP_TRY(hipMemcpyAsync(C, A->d_C, c_elems * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SPARTA_OK;
}

// (the product itself: below, inside this guard and capture scope)
int spmm_run(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int64_t shard_rows, int64_t shard_stride, int32_t n_cols,
             void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, int32_t ptr_space, hipStream_t st, int32_t algo,
             float* dt_ms);

int spmm_impl(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int64_t shard_rows, int64_t shard_stride, int32_t n_cols,
              void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, int32_t ptr_space, void* stream, int32_t algo,
              float* dt_ms) {
    using sparta::fail;
    if (!A || !B || !C) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: NULL argument");
    if (n_cols <= 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: n_cols must be > 0");
    if (b_layout != SPARTA_COL_MAJOR && b_layout != SPARTA_ROW_MAJOR) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: bad b_layout");
    if (c_layout != SPARTA_COL_MAJOR && c_layout != SPARTA_ROW_MAJOR) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: bad c_layout");
    if (shard_rows == 0 && ldb < (b_layout == SPARTA_COL_MAJOR ? A->cols : (int64_t)n_cols))
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: ldb too small");
    if (ldc < (c_layout == SPARTA_COL_MAJOR ? A->rows : (int64_t)n_cols)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: ldc too small");
    if (algo != SPARTA_SPMM_MFMA && algo != SPARTA_SPMM_EXACT) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: bad algo");
    if (ptr_space != SPARTA_PTR_HOST && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm: bad ptr_space");
    // (the 16-bit kernels read B a dword and more at a time, some straight into LDS: an odd-element base is refused like an odd ldb, before anything is launched)
    if (A->dtype != SPARTA_F32 && ptr_space == SPARTA_PTR_DEVICE && ((uintptr_t)B % 4) != 0)
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: 16-bit B must start on a 4-byte boundary (16-byte loads start on 4-byte boundaries)");

    const DeviceCall call{"sparta_vbs_spmm", A, (hipStream_t)stream, ptr_space == SPARTA_PTR_DEVICE, dt_ms, "the product"};
    return open_call(call, [&](hipStream_t st) {
        return spmm_run(A, B, ldb, b_layout, shard_rows, shard_stride, n_cols, C, ldc, c_layout, accumulate, ptr_space, st, algo, dt_ms);
    });
}

// the product of a checked call, inside spmm_impl's guard and capture scope
int spmm_run(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int64_t shard_rows, int64_t shard_stride, int32_t n_cols,
             void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, int32_t ptr_space, hipStream_t st, int32_t algo,
             float* dt_ms) {
    using sparta::fail;
    if (A->dtype != SPARTA_F32)
        return spmm16_impl(A, B, ldb, b_layout, shard_rows, shard_stride, n_cols, C, ldc, c_layout, accumulate, ptr_space, st, algo, dt_ms);

    const float* dB = (const float*)B;
    float* dC = (float*)C;
    const size_t b_elems = (size_t)ldb * (size_t)(b_layout == SPARTA_COL_MAJOR ? n_cols : A->cols);
    const size_t c_elems = (size_t)ldc * (size_t)(c_layout == SPARTA_COL_MAJOR ? n_cols : A->rows);
    if (ptr_space == SPARTA_PTR_HOST) {
        // the reference's back-end contract: host in, host out, dt excludes the copies
        if (int rc = A->d_B.ensure(b_elems * sizeof(float), A->retired)) return rc;
        if (int rc = A->d_C.ensure(c_elems * sizeof(float), A->retired)) return rc;
        HIP_TRY(hipMemcpyAsync(A->d_B, B, b_elems * sizeof(float), hipMemcpyHostToDevice, st));
        if (accumulate) HIP_TRY(hipMemcpyAsync(A->d_C, C, c_elems * sizeof(float), hipMemcpyHostToDevice, st));
        else if (c_elems > 0) HIP_TRY(hipMemsetAsync(A->d_C, 0, c_elems * sizeof(float), st));   // ld padding stays defined
        dB = (const float*)A->d_B;
        dC = (float*)A->d_C;
    }

    struct BrmScope { sparta_vbs_t* a; ~BrmScope() { a->brm_ready = nullptr; a->brm_ld = 0; } } brm_scope{A};     // (the row-major B belongs to this product only)
    A->brm_ready = nullptr; A->brm_ld = 0;
    if (algo == SPARTA_SPMM_EXACT && A->ext_sparse && (A->n_sp_rows > 0 || A->u_steps_total > 0))
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: SPARTA_SPMM_EXACT needs the dense image of every block-row (handle made by sparta_vbs_create_from_csr)");
    if (dt_ms) HIP_TRY(hipEventRecord(A->ev0, st));
    if (algo == SPARTA_SPMM_EXACT) {
        if (int rc = ensure_legacy_image(A, st)) return rc;
        if (A->n_brows > 0) {
            launch_f32_exact((unsigned)A->n_brows, st, A->d_brows, A->d_jab, A->d_A, dB, dC, ldb, ldc, A->cols, (int)n_cols, (int)A->w,
                             (int)(b_layout == SPARTA_ROW_MAJOR), (int)(c_layout == SPARTA_ROW_MAJOR), (int)accumulate, shard_rows, shard_stride);
        }
    } else {
        const char* nv = std::getenv("SPARTA_NO_VEC");
        const bool novec = nv && nv[0] == '1';
        const int n_nt = (n_cols + kTN - 1) / kTN;
        const bool full_slabs = (n_cols % kTN) == 0;
        // two product paths (both branch-free, both need full panels) + the generic fallback for odd shapes
        // The stream kernels address B and C through buffer descriptors with 32-bit byte offsets inside one 128-column slab
        // (range-checked against 2 GB): 127 columns x leading dimension x 4 bytes must stay below 2^31, i.e. ld < 4.2 M
        // elements for the column-major layouts.  Larger leading dimensions take the per-class / generic kernels (64-bit
        // pointer arithmetic).
        const int64_t ld_lim = ((int64_t)1 << 31) / (128 * 4) - 64;
        const bool ld_ok = (b_layout == SPARTA_ROW_MAJOR ? ldb * 32 : ldb * 128) < ((int64_t)1 << 29) - 4096 &&
                           (c_layout == SPARTA_ROW_MAJOR ? ldc * 64 : ldc * 128) < ((int64_t)1 << 29) - 4096;
        (void)ld_lim;
        const bool can_stream = A->n_workers > 0 && full_slabs && !novec && !force_generic() && ld_ok;
        const bool can_class = (A->w % kKP) == 0 && full_slabs && !novec && !force_generic();

        // persistent stream kernel + fix-up of the split tiles
        auto run_stream = [&](float* Cout, bool prof) -> int {
            const size_t slab = (size_t)A->n_slots * SK_SLOT_FLOATS;
            if (A->n_split > 0)
                if (int rc = A->d_ws.ensure(slab * n_nt * sizeof(float), A->retired)) return rc;
            if (shard_rows > 0)
                if (int rc = ensure_gathered_steps(A, shard_rows, st)) return rc;
            // the LDS-staged kernels (33..64-row tiles; any tile under a row-major or gathered B) read the reference-layout image; the no-barrier kernel the fragment image
            if (A->n_steps[1] > 0 || !((A->d_a_frag || A->d_a_pack) && b_layout == SPARTA_COL_MAJOR && shard_rows == 0))
                if (int rc = ensure_legacy_image(A, st)) return rc;
            StreamParams sp;
            sp.A = A->d_A; sp.B = dB; sp.C = Cout; sp.ws = (float*)A->d_ws;
            sp.ldb = ldb; sp.ldc = ldc; sp.cols = A->cols; sp.shard_rows = shard_rows; sp.shard_stride = shard_stride;
            sp.ws_slab_stride = (int64_t)slab; sp.accumulate = accumulate != 0; sp.c_row_major = c_layout == SPARTA_ROW_MAJOR;
            sp.N = n_cols; sp.w = (int32_t)A->w; sp.B_tail = nullptr;
            sp.clk = nullptr;
            sp.stagger = [] { const char* e = std::getenv("SPARTA_STAGGER"); return e ? atoi(e) : 0; }();
            if (A->n_steps[0] + A->n_steps[1] > 0) {
                if (prof) HIP_TRY(hipEventRecord(A->cev[0][0], st));
                if (A->has_tail && shard_rows == 0) {
                    if (int rc = A->d_btail.ensure((size_t)A->w * n_cols * sizeof(float), A->retired)) return rc;
                    const int64_t row0 = ((A->cols - 1) / A->w) * A->w;
                    launch_tail_copy(st, dB, ldb, (int)(b_layout == SPARTA_ROW_MAJOR), row0, A->cols, (int)A->w, (int)n_cols, (float*)A->d_btail);
                    sp.B_tail = (const float*)A->d_btail;
                }
                const dim3 grid((unsigned)A->n_workers, (unsigned)n_nt);
                // heavier type first; the clock probe rides on the launch with more steps
                const int probe_ty = A->n_steps[1] >= A->n_steps[0] ? 1 : 0;
                for (int ty = 1; ty >= 0; ty--) {
                    if (A->n_steps[ty] == 0) continue;
                    sp.steps = shard_rows > 0 ? A->gathered[(size_t)A->g_cur].steps[ty] : A->d_steps[ty]; sp.worker_range = A->d_wrange[ty]; sp.c_nt = c_store_nt(A, ty, sp.C, sp.ldc, sp.c_row_major != 0);
                    sp.clk = (prof && ty == probe_ty) ? A->d_clk : nullptr;
                    if (ty == 0 && (A->d_a_frag || A->d_a_pack) && b_layout == SPARTA_COL_MAJOR && shard_rows == 0) {
                        StreamParams sd = sp;                 // the <= 32-row tiles without the workgroup stage
                        sd.A = A->d_a_pack ? A->d_a_pack : A->d_a_frag;
                        if (A->d_a_pack) { sd.steps = A->d_psteps; sd.worker_range = A->d_pwrange; }      // packed handle: same workers and segments, fewer steps
                        // tiles of arbitrary height + column-major C: finished tiles wait in an LDS ring for whole aligned blocks of 32 rows (k_f32_direct.hip)
                        const int cst = [] { const char* e = std::getenv("SPARTA_CSTAGE"); return e ? atoi(e) : -1; }();     // (read per launch: tests flip it)
                        const bool c_stage = c_layout == SPARTA_COL_MAJOR && (cst >= 0 ? cst != 0 : ring_tiles(A));
                        sd.c_nt = c_store_nt(A, ty, sd.C, sd.ldc, sd.c_row_major != 0, c_stage);
                        if (A->d_a_pack) launch_f32_packed(c_stage, grid, st, sd);
                        else launch_f32_direct(c_stage, grid, st, sd);
                    } else launch_f32_stream(ty != 0, b_layout == SPARTA_ROW_MAJOR, shard_rows > 0, grid, st, sp);
                }
                if (prof) { HIP_TRY(hipEventRecord(A->cev[0][1], st)); A->class_ran[0] = true; }
            }
            const bool fix_launch = A->n_fix > 0 && !(accumulate && A->n_split == 0);   // C += 0 for the block-rows without blocks: nothing to launch
            const bool zero_launch = !A->zero_ranges.empty() && !accumulate;
            if (fix_launch || zero_launch) {
                if (prof) HIP_TRY(hipEventRecord(A->cev[1][0], st));
                if (fix_launch && A->n_big_fix > 0)
                    launch_fixup_group(dim3((unsigned)A->n_big_fix, (unsigned)n_nt, (unsigned)((A->max_tile_slots + kFixGroup - 1) / kFixGroup)), st, A->d_fix,
                                       A->d_big_fix, A->d_fix_slots, (float*)A->d_ws, (int64_t)slab);
                if (fix_launch)
                    launch_fixup(dim3((unsigned)A->n_fix, (unsigned)n_nt), st, A->d_fix, A->d_fix_slots, (const float*)A->d_ws, (int64_t)slab, Cout, ldc,
                                 (int)(c_layout == SPARTA_ROW_MAJOR), (int)(accumulate != 0));
                if (zero_launch) launch_zero_ranges(A, Cout, ldc, c_layout == SPARTA_ROW_MAJOR, n_cols, st);
                if (prof) { HIP_TRY(hipEventRecord(A->cev[1][1], st)); A->class_ran[1] = true; }
            }
            return SPARTA_OK;
        };
        // one launch per tile class (<=16 / <=32 / <=64 rows), one workgroup per tile
        auto run_class = [&](float* Cout, bool generic, bool prof) -> int {
            if (int rc = ensure_legacy_image(A, st)) return rc;
            SpmmParams p;
            p.jab = A->d_jab; p.A = A->d_A; p.B = dB; p.C = Cout; p.ldb = ldb; p.ldc = ldc; p.cols = A->cols;
            p.n_ntiles = n_nt; p.N = n_cols; p.w = (int32_t)A->w;
            p.b_row_major = b_layout == SPARTA_ROW_MAJOR; p.c_row_major = c_layout == SPARTA_ROW_MAJOR;
            p.accumulate = accumulate != 0;
            p.shard_rows = shard_rows; p.shard_stride = shard_stride;
            p.vec_ok = novec ? 0 : 1;
            for (int c = 3; c >= 0; c--) {              // heavy classes first
                if (A->n_tiles[c] == 0) continue;
                if (A->n_tiles[c] * (int64_t)p.n_ntiles > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm: grid too large");
                p.tiles = A->d_tiles[c]; p.n_tiles = (int32_t)A->n_tiles[c];
                p.clk = prof ? A->d_clk + 4 * c : nullptr;
                if (prof) HIP_TRY(hipEventRecord(A->cev[c][0], st));
                launch_f32_class(c, p.b_row_major != 0, generic, p, st);
                if (prof) { HIP_TRY(hipEventRecord(A->cev[c][1], st)); A->class_ran[c] = true; }
            }
            return SPARTA_OK;
        };

        // ---- choose the path: forced by SPARTA_PATH, else measured once per (n_cols, layouts, gathered) on this handle -------
        int path = 3;                                   // 1 stream, 2 per-class fast, 3 generic
        const char* pe = std::getenv("SPARTA_PATH");
        const std::string forced = pe ? pe : "auto";
        if (forced == "stream") path = can_stream ? 1 : 3;
        else if (forced == "class") path = can_class ? 2 : 3;
        else if (forced == "generic") path = 3;
        else if (can_stream && can_class) {
            const int64_t key = ((int64_t)n_cols << 8) | (b_layout << 2) | (c_layout << 1) | (shard_rows > 0 ? 1 : 0);
            path = 0;
            for (const auto& kv : A->tuned) if (kv.first == key) path = kv.second;
            if (path == 0 && g_capturing) return capture_refusal("time its two product paths");
            if (path == 0) {
                // plan-time autotune: both paths write a scratch C (the caller's C must not be accumulated into twice)
                if (int rc = A->d_tune.ensure(c_elems * sizeof(float), A->retired)) return rc;
                float best[3] = {0.0f, 1e30f, 1e30f};
                for (int cand = 1; cand <= 2; cand++) {
                    for (int rep = 0; rep < 4; rep++) {
                        HIP_TRY(hipEventRecord(A->tev0, st));
                        if (int rc = cand == 1 ? run_stream((float*)A->d_tune, false) : run_class((float*)A->d_tune, false, false)) return rc;
                        HIP_TRY(hipEventRecord(A->tev1, st));
                        HIP_TRY(hipEventSynchronize(A->tev1));
                        float ms = 0.0f;
                        HIP_TRY(hipEventElapsedTime(&ms, A->tev0, A->tev1));
                        if (rep > 0) best[cand] = std::min(best[cand], ms);
                    }
                }
                path = best[1] <= best[2] ? 1 : 2;
                A->tuned.emplace_back(key, path);
                A->tune_ms[0] = best[1]; A->tune_ms[1] = best[2];
            }
        } else if (can_stream) path = 1;
        else if (can_class) path = 2;

        const bool prof = A->class_timing;
        for (int c = 0; c < 4; c++) A->class_ran[c] = false;
        if (path == 1) { if (int rc = run_stream(dC, prof)) return rc; }
        else if (int rc = run_class(dC, path == 3, prof)) return rc;
        A->last_path = path;
        // one image of A, not two: the no-barrier kernel carries this handle's products (every tile is in the fragment image) -- see ensure_legacy_image
        if (path == 1 && b_layout == SPARTA_COL_MAJOR && shard_rows == 0) drop_legacy_image(A);

        // ---- the sparse rows.  Fully sparse block-rows (flag 1) own their rows of C; rows of MIXED block-rows (flag 2, bit 31 of crow) ADD to what
        // the tile and fix-up launches stored: this launch must stay BEHIND those launches on the same stream (moving the sparse leg to a side
        // stream for overlap needs an event wait for the mixed rows) ----
        // ---- the column-compacted tiles (fp32 handles made from a CSR): they store every row of their block-rows; those block-rows' sparse rows add, below ----
        if (A->u_steps_total > 0) {
            const bool rec = prof && !A->class_ran[2];
            if (rec) HIP_TRY(hipEventRecord(A->cev[2][0], st));
            if (int rc = launch_union_tiles(A, dB, ldb, b_layout == SPARTA_ROW_MAJOR, shard_rows, shard_stride, n_cols, dC, ldc, c_layout == SPARTA_ROW_MAJOR,
                                            accumulate != 0, st)) return rc;
            if (rec) { HIP_TRY(hipEventRecord(A->cev[2][1], st)); A->class_ran[2] = true; }
        }
        if (A->n_sp_rows > 0) {
            if (prof) HIP_TRY(hipEventRecord(A->cev[3][0], st));
            if (int rc = launch_sparse_rows(A, dB, ldb, b_layout == SPARTA_ROW_MAJOR, shard_rows, shard_stride, 0, n_cols, dC, ldc,
                                            c_layout == SPARTA_ROW_MAJOR, accumulate != 0, st)) return rc;
            if (prof) { HIP_TRY(hipEventRecord(A->cev[3][1], st)); A->class_ran[3] = true; }
        }
    }
    HIP_TRY(hipGetLastError());
    if (dt_ms) {
        HIP_TRY(hipEventRecord(A->ev1, st));
        HIP_TRY(hipEventSynchronize(A->ev1));
        HIP_TRY(hipEventElapsedTime(dt_ms, A->ev0, A->ev1));
    }
    if (ptr_space == SPARTA_PTR_HOST) {
        HIP_TRY(hipMemcpyAsync(C, A->d_C, c_elems * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SPARTA_OK;
}

}  // namespace

extern "C" {

int sparta_vbs_spmm(sparta_vbs_t* A, const void* B, int64_t ldb, int32_t b_layout, int32_t n_cols, void* C, int64_t ldc,
                    int32_t c_layout, int32_t accumulate, int32_t ptr_space, void* stream, int32_t algo, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return spmm_impl(A, B, ldb, b_layout, 0, 0, n_cols, C, ldc, c_layout, accumulate, ptr_space, stream, algo, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_spmm")
}

int sparta_vbs_spmm_gathered_ld(sparta_vbs_t* A, const void* B_gathered, int64_t shard_rows, int64_t shard_ld, int64_t shard_stride, int32_t n_cols,
                                void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream, int32_t algo, float* dt_ms) {
    using sparta::fail;
    if (!A) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: NULL handle");
    if (shard_rows <= 0 || shard_rows % A->w != 0)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: shard_rows must be a positive multiple of block_col_size");
    if (shard_ld < shard_rows) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: shard_ld must be >= shard_rows");
    if (shard_stride < shard_ld * (int64_t)(n_cols - 1) + shard_rows) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: shard_stride too small");
    if (A->cols % shard_rows != 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: cols must be n_shards * shard_rows");
    SPARTA_GUARD_BEGIN
    return spmm_impl(A, B_gathered, shard_ld, SPARTA_COL_MAJOR, shard_rows, shard_stride, n_cols, C, ldc, c_layout, accumulate,
                     SPARTA_PTR_DEVICE, stream, algo, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_spmm_gathered")
}

int sparta_vbs_spmm_gathered(sparta_vbs_t* A, const void* B_gathered, int64_t shard_rows, int64_t shard_stride, int32_t n_cols,
                             void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream, int32_t algo, float* dt_ms) {
    if (shard_rows > 0 && shard_stride < shard_rows * (int64_t)n_cols) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_gathered: shard_stride too small");
    return sparta_vbs_spmm_gathered_ld(A, B_gathered, shard_rows, shard_rows, shard_stride, n_cols, C, ldc, c_layout, accumulate, stream, algo, dt_ms);
}

// ---- a B that does not change between products, prepared once ------------------------------------------------------------
struct sparta_b {
    const void* B = nullptr;
    int64_t ldb = 0, shard_rows = 0, shard_stride = 0, cols = 0;
    int32_t n_cols = 0, dtype = 0, device = 0;
    DevBuf<uint8_t> d_Brm;                 // row-major copy for the sparse-row kernels and the column-compacted tiles (nullptr: this handle / shape does not need one)
    int64_t ld_brm = 0;                    // its row stride in elements (n_cols rounded up to 16 bytes)
};

int sparta_vbs_prepare_b(sparta_vbs_t* A, const void* B, int64_t ldb, int64_t shard_rows, int64_t shard_stride, int32_t n_cols, void* stream,
                         sparta_b_t** out) {
    using sparta::fail;
    SPARTA_GUARD_BEGIN
    if (!A || !B || !out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_prepare_b: NULL argument");
    *out = nullptr;
    if (n_cols <= 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_prepare_b: n_cols must be > 0");
    if (shard_rows == 0 && ldb < A->cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_prepare_b: ldb too small");
    // a gathered B: `ldb` is the column stride inside a slab (sparta_vbs_spmm_gathered_ld's shard_ld; 0 = unpadded, shard_rows)
    const int64_t shard_ld = shard_rows != 0 ? (ldb > 0 ? ldb : shard_rows) : 0;
    if (shard_rows != 0 && (shard_rows < 0 || shard_rows % A->w != 0 || A->cols % shard_rows != 0 || shard_ld < shard_rows ||
                            shard_stride < shard_ld * (int64_t)(n_cols - 1) + shard_rows))
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_prepare_b: bad gathered layout");
    if (A->dtype != SPARTA_F32 && ((uintptr_t)B % 4) != 0)          // (as sparta_vbs_spmm refuses it: the copy made below and every later product read B a dword and more at a time)
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_prepare_b: 16-bit B must start on a 4-byte boundary");
    if (g_capturing) return capture_refusal("prepare a copy of B");
    DeviceGuard guard(A->device);
    // owned by `hold` until it is handed to the caller (the guard above outlives it: the copy is freed with the handle's device current)
    std::unique_ptr<sparta_b> hold(new (std::nothrow) sparta_b);
    sparta_b* p = hold.get();
    if (!p) return fail(SPARTA_ERR_ALLOC, "sparta_vbs_prepare_b: out of host memory");
    p->B = B; p->ldb = shard_rows ? shard_ld : ldb; p->shard_rows = shard_rows; p->shard_stride = shard_stride; p->cols = A->cols;
    p->n_cols = n_cols; p->dtype = A->dtype; p->device = A->device;
    const size_t esz = A->dtype == SPARTA_F32 ? 4 : 2;
    // the sparse-row kernels of this handle would transpose this B per product (launch_sparse_rows: not when a handful of rows reads it in place)
    // (nor when the resident-column kernel carries the products of a plain column-major B: it reads the columns where they are; a later product into a ROW-major C
    // then transposes per call as sparta_vbs_spmm does)
    const bool needs_copy = (A->n_sp_rows > 0 && !(A->sp_nnz * 8 < A->cols) && !(A->cr_slices > 0 && shard_rows == 0)) || A->u_steps_total > 0;
    if (needs_copy) {
        hipStream_t st = (hipStream_t)stream;
        const int64_t n_wg = ((A->cols + 63) / 64) * (int64_t)((n_cols + 63) / 64);
        if (n_wg > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_prepare_b: B too large for the transpose grid");
        const int64_t per16 = 16 / (int64_t)esz;
        p->ld_brm = (n_cols + per16 - 1) / per16 * per16;
        if (p->d_Brm.alloc((size_t)A->cols * (size_t)p->ld_brm * esz) != hipSuccess) return fail(SPARTA_ERR_ALLOC, "sparta_vbs_prepare_b: out of device memory");
        launch_b_to_row_major(A->dtype != SPARTA_F32, (unsigned)n_wg, st, B, p->ldb, shard_rows, shard_stride, A->cols, (int)n_cols, p->d_Brm, p->ld_brm);
        if (hipGetLastError() != hipSuccess) return fail(SPARTA_ERR_HIP, "sparta_vbs_prepare_b: launch failed");
    }
    *out = hold.release();
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_prepare_b")
}

int sparta_vbs_spmm_prepared(sparta_vbs_t* A, const sparta_b_t* Bp, void* C, int64_t ldc, int32_t c_layout, int32_t accumulate, void* stream,
                             float* dt_ms) {
    using sparta::fail;
    if (!A || !Bp || !C) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_prepared: NULL argument");
    if (Bp->cols != A->cols || Bp->dtype != A->dtype || Bp->device != A->device)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_prepared: this B was prepared for another handle shape / type / device");
    SPARTA_GUARD_BEGIN
    // (cleared on every way out, exceptions included: a stale pointer would make a later plain product gather from this B)
    struct Prepared { sparta_vbs_t* a; ~Prepared() { a->prepared_brm = nullptr; a->prepared_ld = 0; } } guard{A};
    A->prepared_brm = Bp->d_Brm; A->prepared_ld = Bp->ld_brm;
    return spmm_impl(A, Bp->B, Bp->ldb, SPARTA_COL_MAJOR, Bp->shard_rows, Bp->shard_stride, Bp->n_cols, C, ldc, c_layout, accumulate,
                     SPARTA_PTR_DEVICE, stream, SPARTA_SPMM_MFMA, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_spmm_prepared")
}

int sparta_b_destroy(sparta_b_t* Bp) {
    if (!Bp) return SPARTA_OK;
    DeviceGuard guard(Bp->device);
    delete Bp;
    return SPARTA_OK;
}

int sparta_vbs_set_class_timing(sparta_vbs_t* A, int32_t enable) {
    using sparta::fail;
    if (!A) return fail(SPARTA_ERR_INVALID, "sparta_vbs_set_class_timing: NULL handle");
    DeviceGuard guard(A->device);
    if (enable && !A->cev[0][0]) {
        for (int c = 0; c < 4; c++)
            for (int e = 0; e < 2; e++) HIP_TRY(A->cev[c][e].create());
    }
    if (enable && !A->d_clk) {
        HIP_TRY(A->d_clk.alloc(16 + 4 * 64 * 8 + 2048));
        HIP_TRY(hipMemset(A->d_clk, 0, (16 + 4 * 64 * 8 + 2048) * sizeof(long long)));
    }
    A->class_timing = enable != 0;
    return SPARTA_OK;
}

int sparta_vbs_class_times(sparta_vbs_t* A, float* ms_out) {
    using sparta::fail;
    if (!A || !ms_out) return fail(SPARTA_ERR_INVALID, "sparta_vbs_class_times: NULL argument");
    DeviceGuard guard(A->device);
    for (int c = 0; c < 4; c++) {
        ms_out[c] = 0.0f;
        if (!A->class_timing || !A->class_ran[c]) continue;
        HIP_TRY(hipEventSynchronize(A->cev[c][1]));
        HIP_TRY(hipEventElapsedTime(&ms_out[c], A->cev[c][0], A->cev[c][1]));
    }
    return SPARTA_OK;
}

int sparta_pack_blocks(const void* src, int64_t block_bytes, const int32_t* ids_dev, int64_t n_blocks, void* dst, void* stream) {
    using sparta::fail;
    if (n_blocks < 0 || block_bytes <= 0 || block_bytes % 16 != 0)
        return fail(SPARTA_ERR_INVALID, "sparta_pack_blocks: block_bytes must be a positive multiple of 16, n_blocks >= 0");
    if (n_blocks == 0) return SPARTA_OK;
    if (!src || !ids_dev || !dst) return fail(SPARTA_ERR_INVALID, "sparta_pack_blocks: NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) % 16 != 0) return fail(SPARTA_ERR_INVALID, "sparta_pack_blocks: src and dst must be 16-byte aligned");
    if (n_blocks > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_pack_blocks: too many blocks for one launch");
    const int64_t vec = block_bytes / 16;
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8, vec / (4 * kThreads)));
    launch_pack_blocks(dim3((unsigned)n_blocks, gy), (hipStream_t)stream, src, ids_dev, dst, vec);
    HIP_TRY(hipGetLastError());
    return SPARTA_OK;
}

}  // extern "C"

// ---- SDDMM (k_sddmm.hip) ----------------------------------------------------------------------------------------------------------------
namespace {

// the work list: per block-row with stored blocks, per tile of <= 32 of its rows, its groups of 32 stored columns in runs of <= kSdGroups
// (built on the host from the block-row descriptors the handle already holds, at the first call)
int ensure_sddmm_items(sparta_vbs_t* A) {
    using sparta::fail;
    if (A->n_sd_items >= 0) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload its work list", "sparta_vbs_sddmm");
    std::vector<BlockRowDesc> brows((size_t)A->n_brows);
    if (A->n_brows > 0) HIP_TRY(hipMemcpy(brows.data(), A->d_brows, brows.size() * sizeof(BlockRowDesc), hipMemcpyDeviceToHost));
    std::vector<SddmmItem> items;
    for (int64_t ib = 0; ib < A->n_brows; ib++) {
        const BlockRowDesc& br = brows[(size_t)ib];
        const int64_t n_groups = ((int64_t)br.nb * A->w + 31) / 32;
        for (int32_t r0 = 0; r0 < br.h; r0 += 32)
            for (int64_t g0 = 0; g0 < n_groups; g0 += kSdGroups)
                items.push_back(SddmmItem{(int32_t)ib, r0, (int32_t)g0, (int32_t)std::min<int64_t>(kSdGroups, n_groups - g0)});
    }
    if ((int64_t)items.size() > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_sddmm: more than 2^31 - 1 work items");
    if (!items.empty()) HIP_TRY(A->d_sd_items.upload(items));
    A->n_sd_items = (int64_t)items.size();
    return SPARTA_OK;
}

int sddmm_impl(sparta_vbs_t* A, const void* X, int64_t ldx, const void* Y, int64_t ldy, int32_t k, float* G, int32_t accumulate, int32_t ptr_space,
               void* stream, float* dt_ms) {
    using sparta::fail;
    if (!A || !X || !Y || !G) return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: NULL argument");
    if (k <= 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: k must be > 0");
    if (ptr_space != SPARTA_PTR_HOST && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: bad ptr_space");
    if (ldx < A->rows || ldy < A->cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: ldx < rows or ldy < cols");
    if (ldx > (INT64_C(1) << 61) / k || ldy > (INT64_C(1) << 61) / k) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_sddmm: ldx * k or ldy * k beyond 2^61");
    const bool h16 = A->dtype != SPARTA_F32;
    if (h16 && ptr_space == SPARTA_PTR_DEVICE && ((ldx | ldy) & 1)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: 16-bit handles need even ldx, ldy");
    if (h16 && ptr_space == SPARTA_PTR_DEVICE && (((uintptr_t)X | (uintptr_t)Y) % 4) != 0)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_sddmm: 16-bit X and Y must start on 4-byte boundaries");
    if (A->ext_sparse)
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_sddmm: the handle does not hold the dense blocks of every block-row (made by sparta_vbs_create_from_csr)");

    const DeviceCall call{"sparta_vbs_sddmm", A, (hipStream_t)stream, ptr_space == SPARTA_PTR_DEVICE, dt_ms, "the product", A->ev0, A->ev1};
    return open_call(call, [&](hipStream_t st) -> int {
        if (int rc = ensure_sddmm_items(A)) return rc;

        const void* dX = X;
        const void* dY = Y;
        float* dG = G;
        int64_t kx = ldx, ky = ldy;
        const size_t x_elems = (size_t)ldx * (size_t)(k - 1) + (size_t)A->rows, y_elems = (size_t)ldy * (size_t)(k - 1) + (size_t)A->cols;
        const size_t g_elems = (size_t)A->nztot;
        if (ptr_space == SPARTA_PTR_HOST) {
            // host in, host out: X, Y, G staged in one device buffer; 16-bit handles round X, Y on the device
            if (int rc = A->d_sd_ws.ensure((x_elems + y_elems + g_elems) * sizeof(float), A->retired)) return rc;
            float* ws = (float*)A->d_sd_ws;
            HIP_TRY(hipMemcpyAsync(ws, X, x_elems * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ws + x_elems, Y, y_elems * sizeof(float), hipMemcpyHostToDevice, st));
            if (accumulate && g_elems > 0) HIP_TRY(hipMemcpyAsync(ws + x_elems + y_elems, G, g_elems * sizeof(float), hipMemcpyHostToDevice, st));
            dX = ws; dY = ws + x_elems; dG = ws + x_elems + y_elems;
            if (h16) {
                kx = (A->rows + 7) / 8 * 8; ky = (A->cols + 7) / 8 * 8;       // (multiples of 8: the 16-byte loads of k_sddmm.hip)
                const size_t hx = (size_t)kx * (size_t)k, hy = (size_t)ky * (size_t)k;
                if (int rc = A->d_sd_h16.ensure((hx + hy) * sizeof(uint16_t), A->retired)) return rc;
                uint16_t* hw = (uint16_t*)A->d_sd_h16;
                launch_convert_h16(A->dtype == SPARTA_BF16, st, ws, ldx, A->rows, k, hw, kx);
                launch_convert_h16(A->dtype == SPARTA_BF16, st, ws + x_elems, ldy, A->cols, k, hw + hx, ky);
                HIP_TRY(hipGetLastError());
                dX = hw; dY = hw + hx;
            }
        }
        SddmmParams p;
        p.brows = A->d_brows; p.jab = A->d_jab; p.items = A->d_sd_items;
        p.X = dX; p.Y = dY; p.G = dG;
        p.ldx = kx; p.ldy = ky; p.cols = A->cols;
        p.k = k; p.w = (int32_t)A->w; p.accumulate = accumulate != 0; p.pad = 0;
        const int trc = timed_launches(call, [&](hipStream_t) {
            if (A->live_on) {
                // a live set is installed: the dead blocks get their zeros (accumulate = 0) from the mask kernel and the snapshot, in front; the live kernel walks the
                // compacted group lists over the same grid (an item past its block-row's live groups returns at once), so nothing here depends on a count read back
                if (!p.accumulate && A->n_prune > 0 && A->nztot > 0) launch_mask_blocks(st, A->d_prune, A->n_prune, A->d_live_keep, dG, nullptr, nullptr, nullptr);
                launch_sddmm_live(A->dtype, (unsigned)A->n_sd_items, st, p, SddmmLive{A->d_live_groups, A->d_live_goff, A->d_live_gcount, A->d_live_keep});
            } else {
                launch_sddmm(A->dtype, (unsigned)A->n_sd_items, st, p);
            }
        });
        if (trc) return trc;
        if (ptr_space == SPARTA_PTR_HOST) {
            if (g_elems > 0) HIP_TRY(hipMemcpyAsync(G, dG, g_elems * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return SPARTA_OK;
    });
}

}  // namespace

extern "C" int sparta_vbs_sddmm(sparta_vbs_t* A, const void* X, int64_t ldx, const void* Y, int64_t ldy, int32_t k, float* G, int32_t accumulate,
                                int32_t ptr_space, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return sddmm_impl(A, X, ldx, Y, ldy, k, G, accumulate, ptr_space, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_sddmm")
}

// ---- sparta_vbs_set_values (k_update.hip) -----------------------------------------------------------------------------------------------
namespace {

// every device image of an updatable handle written from `src` (nztot floats in the mab layout, device memory): the launches of sparta_vbs_set_values, which
// sparta_vbs_sgd_step repeats behind its elementwise kernel.  Returns the number of launches.
// the fp8 image behind a write of values (sparta_vbs_set_forward_a8): while the switch is on, one launch of the quantise kernel on the array the images were
// just written from, in stream order.  Launches only: capturable, and a replay requantises.
// the fp8 image with a live-block set (sparta_vbs_set_a8_live): the exponent words of the private records into the compacted records the product walks, one
// launch in stream order behind whatever moved either of them (a compaction rewrites every position from the plain records, a quantise launch every exponent)
void a8_live_place_scales(sparta_vbs_t* A, hipStream_t st) {
    if (!A->a8_live || !A->a8_on || !A->a8_built || A->a8_ty < 0 || !A->live_fwd_built || A->live_fwd_ty != A->a8_ty) return;
    const int ty = A->a8_ty;
    launch_a8_live_scales(st, A->d_a8_steps, A->n_steps[ty], A->upd_base[ty], (int64_t)(ty ? 64 : 32) * A->kp16, A->d_fwd_steps);
    A->a8_live_launches++;
}

void a8_requantize(sparta_vbs_t* A, hipStream_t st, const float* src) {
    if (!A->a8_on || !A->a8_built || A->a8_ty < 0 || A->nztot <= 0) return;
    const int ty = A->a8_ty;
    launch_a8_quantize(ty ? 64 : 32, A->kp16, st, A->d_upd_map[ty], A->n_steps[ty], src, A->d_a8 + A->upd_base[ty], A->d_a8_steps);
    A->a8_valid = true;
    A->a8_launches++;
    a8_live_place_scales(A, st);
}

int launch_images_from(sparta_vbs_t* A, hipStream_t st, const float* src) {
    int launches = 0;
    if (A->dtype == SPARTA_F32) {
        // the fragment image holds every stored element when the handle has no 33..64-row tiles: its kernel then writes the reference-layout image (if the
        // handle still holds it: a dropped one is rebuilt from the fragment image when a call asks for it) from the same read of mab
        const bool frag = A->d_a_frag != nullptr && A->n_steps[0] > 0;
        const bool frag_covers = frag && A->n_steps[1] == 0;
        if (A->d_A && !frag_covers) { launch_update_copy(st, src, A->nztot, A->d_A); launches++; }
        if (frag) { launch_update_f32_frag(st, A->d_steps[0], A->n_steps[0], src, A->d_a_frag, frag_covers ? A->d_A : nullptr); launches++; }
    } else {
        const bool bf16 = A->dtype == SPARTA_BF16;
        for (int ty = 0; ty < 2; ty++)
            if (A->n_steps[ty] > 0) {
                launch_update_h16(bf16, false, ty ? 64 : 32, A->kp16, st, A->d_upd_map[ty], A->n_steps[ty], src, (uint16_t*)A->d_A.get() + A->upd_base[ty]);
                launches++;
            }
        if (A->n_upd_hub > 0) { launch_update_h16(bf16, true, 64, 64, st, A->d_upd_hub, A->n_upd_hub, src, A->d_hub_A); launches++; }
        if (A->n_t_src > 0) { launch_update_h16_t(bf16, st, A->d_t_src, A->n_t_src, (int)A->w, src, A->d_t_A); launches++; }      // the image of sparta_vbs_spmm_t
    }
    return launches;
}

int set_values_impl(sparta_vbs_t* A, const float* mab, int32_t ptr_space, void* stream, float* dt_ms) {
    using sparta::fail;
    if (!A) return fail(SPARTA_ERR_INVALID, "sparta_vbs_set_values: NULL handle");
    if (!mab && A->nztot > 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_set_values: mab is NULL");
    if (ptr_space != SPARTA_PTR_HOST && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_set_values: bad ptr_space");
    if (!(A->create_flags & SPARTA_CREATE_UPDATABLE)) return not_updatable("sparta_vbs_set_values");
    const DeviceCall call{"sparta_vbs_set_values", A, (hipStream_t)stream, ptr_space == SPARTA_PTR_DEVICE, dt_ms, "the update", A->ev0, A->ev1, A->nztot <= 0};
    return open_call(call, [&](hipStream_t st) -> int {
        const float* src = mab;
        if (ptr_space == SPARTA_PTR_HOST && A->nztot > 0) {
            if (int rc = A->d_upd_ws.ensure((size_t)A->nztot * sizeof(float), A->retired)) return rc;
            HIP_TRY(hipMemcpyAsync(A->d_upd_ws, mab, (size_t)A->nztot * sizeof(float), hipMemcpyHostToDevice, st));
            src = (const float*)A->d_upd_ws;
        }
        if (int rc = timed_launches(call, [&](hipStream_t) { (void)launch_images_from(A, st, src); a8_requantize(A, st, src); })) return rc;
        if (ptr_space == SPARTA_PTR_HOST) HIP_TRY(hipStreamSynchronize(st));          // (the caller's array is free again when the call returns)
        return SPARTA_OK;
    });
}

}  // namespace

extern "C" int sparta_vbs_set_values(sparta_vbs_t* A, const float* mab, int32_t ptr_space, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return set_values_impl(A, mab, ptr_space, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_set_values")
}

// ---- sparta_vbs_sgd_step (k_update.hip) ---------------------------------------------------------------------------------------------------
namespace {

// Which image kernel may own the arithmetic of a step: the one whose image holds every stored element exactly once.  Plan data only:
//   fp32    the fragment image, when the handle has no 33..64-row tiles (what lets set_values write d_A from the fragment kernel's own read): the rows
//           m < mt of the steps of a block-row's <= 32-row tiles partition its stored elements, upd_cover[0] == nztot says no block-row is outside
//   16-bit  the slices of ONE stream image (build_stream_plans: a block-row is in exactly one of the <= 32-row tiles, the 33..64-row / pair tiles, the hub
//           plan, and the steps of its tiles partition its elements), when the other stream image and the hub image are empty
// Returns the tile type of that image, -1 for the two-pass form.
int sgd_fused_image(const sparta_vbs_t* A) {
    if (A->dtype == SPARTA_F32) return (A->d_a_frag != nullptr && A->n_steps[0] > 0 && A->n_steps[1] == 0 && A->upd_cover[0] == A->nztot) ? 0 : -1;
    if (A->n_upd_hub > 0) return -1;
    for (int ty = 0; ty < 2; ty++)
        if (A->n_steps[ty] > 0 && A->n_steps[1 - ty] == 0 && A->d_upd_map[ty] != nullptr && A->upd_cover[ty] == A->nztot) return ty;
    return -1;
}

// Whether a step asks for the image kernel (sgd_fused_image then says whether the handle has one).  By default every step does: on the headline handle the
// image kernel measured faster than the elementwise kernel + the set_values launches, and than the same update as torch ops + set_values, with and without
// momentum, fp32 and f16.  SPARTA_SGD_FUSE=0 asks for the two-pass form on every step, 1 is the default spelled out.  Read at every
// call through env_switch (no plan depends on it): scripts/sgd_step_record.py and the tests drive both forms of one handle in one process.
// Live steps (sparta_vbs_set_live_steps): the switch counts only while a live set is installed; read when a step is called or captured.  The image kernels'
// words exist then: the enabling call built them, and every set_live_blocks since rewrote them behind the snapshot.
bool live_steps_active(const sparta_vbs_t* A) { return A->live_on && A->live_steps && A->live_steps_built; }

// entry: the name the messages carry.  R: the control record of sparta_vbs_sgd_step_ctl, or NULL (the step as it always was)
int sgd_step_impl(const char* entry, sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, const void* R, void* stream, float* dt_ms) {
    const auto fail = [entry](int code, const char* what) { return sparta::fail(code, std::string(entry) + what); };
    if (!A) return fail(SPARTA_ERR_INVALID, ": NULL handle");
    if (A->nztot > 0 && (!W || !G || !cfg)) return fail(SPARTA_ERR_INVALID, ": W, G or cfg is NULL");
    if (cfg && cfg->momentum != 0.0f && !M) return fail(SPARTA_ERR_INVALID, ": M is NULL with momentum != 0");
    if (!(A->create_flags & SPARTA_CREATE_UPDATABLE)) return not_updatable(entry);
    if ((uintptr_t)R % 8 != 0) return fail(SPARTA_ERR_INVALID, ": the control record R must be 8-byte aligned");
    int launches = 0;
    int fused = -1;
    bool live = false;
    const DeviceCall call{entry, A, (hipStream_t)stream, true, dt_ms, "the step", A->ev0, A->ev1, A->nztot <= 0};
    const int rc = device_call(call, [&](hipStream_t st) {
        const SgdCfg c{cfg->lr, cfg->momentum, cfg->weight_decay, cfg->grad_scale};
        const uint32_t* ctl = (const uint32_t*)R;
        if (env_switch("SPARTA_SGD_FUSE")) fused = sgd_fused_image(A);
        live = live_steps_active(A);
        if (fused >= 0 && A->dtype == SPARTA_F32) {
            if (live) launch_sgd_f32_frag_live(st, A->d_steps[0], A->n_steps[0], W, G, M, c, ctl, A->d_a_frag, A->d_A, A->d_live_words);
            else launch_sgd_f32_frag(st, A->d_steps[0], A->n_steps[0], W, G, M, c, ctl, A->d_a_frag, A->d_A);
            launches = 1;
        } else if (fused >= 0) {
            const bool bf16 = A->dtype == SPARTA_BF16;
            uint16_t* dst = (uint16_t*)A->d_A.get() + A->upd_base[fused];
            if (live) launch_sgd_h16_live(bf16, fused ? 64 : 32, A->kp16, st, A->d_upd_map[fused], A->n_steps[fused], W, G, M, c, ctl, dst, A->d_live_words);
            else launch_sgd_h16(bf16, fused ? 64 : 32, A->kp16, st, A->d_upd_map[fused], A->n_steps[fused], W, G, M, c, ctl, dst);
            launches = 1;
            if (A->n_t_src > 0) { launch_update_h16_t(bf16, st, A->d_t_src, A->n_t_src, (int)A->w, W, A->d_t_A); launches++; }   // reads the W written above
        } else {
            if (live) launch_sgd_blocks_live(st, A->d_prune, A->n_prune, A->d_live_keep, W, G, M, c, ctl);
            else launch_sgd_step(st, A->nztot, W, G, M, c, ctl);
            launches = 1 + launch_images_from(A, st, W);
        }
        a8_requantize(A, st, W);                  // (a step the control record skipped left W as it was: the image comes out as it stood)
    });
    if (rc) return rc;
    A->step_last_live = live ? 1 : 0;
    A->step_last_fused = fused >= 0 ? 1 : 0;
    A->step_last_launches = launches;
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_vbs_sgd_step(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return sgd_step_impl("sparta_vbs_sgd_step", A, W, G, M, cfg, nullptr, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_sgd_step")
}

extern "C" int sparta_vbs_sgd_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, const void* R, void* stream,
                                       float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return sgd_step_impl("sparta_vbs_sgd_step_ctl", A, W, G, M, cfg, R, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_sgd_step_ctl")
}

// ---- sparta_vbs_adam_step (k_update.hip) --------------------------------------------------------------------------------------------------
namespace {

// Whether a step asks for the image kernel (sgd_fused_image says whether the handle has one): the default is the form that measured faster on the headline
// handle, DESIGN.md section 3.8.  SPARTA_ADAM_FUSE=0 asks for the two-pass form on every step, 1 for the image kernel wherever the handle has one.  Read at
// every call through env_switch, as SPARTA_SGD_FUSE is.
int adam_step_impl(const char* entry, sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S, const sparta_adam_cfg* cfg, const void* R, void* stream,
                   float* dt_ms) {
    const auto fail = [entry](int code, const char* what) { return sparta::fail(code, std::string(entry) + what); };
    if (!A) return fail(SPARTA_ERR_INVALID, ": NULL handle");
    if (A->nztot > 0 && (!W || !G || !M || !V || !S || !cfg)) return fail(SPARTA_ERR_INVALID, ": W, G, M, V, S or cfg is NULL");
    if (cfg) {
        if (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f))
            return fail(SPARTA_ERR_INVALID, ": beta1 and beta2 must lie in [0, 1)");
        if (!(cfg->eps > 0.0f)) return fail(SPARTA_ERR_INVALID, ": eps must be > 0");
        if (cfg->reserved != 0) return fail(SPARTA_ERR_INVALID, ": cfg->reserved must be 0");
    }
    if (!(A->create_flags & SPARTA_CREATE_UPDATABLE)) return not_updatable(entry);
    if ((uintptr_t)R % 8 != 0) return fail(SPARTA_ERR_INVALID, ": the control record R must be 8-byte aligned");
    int launches = 0;
    int fused = -1;
    bool live = false;
    const DeviceCall call{entry, A, (hipStream_t)stream, true, dt_ms, "the step", A->ev0, A->ev1, A->nztot <= 0};
    const int rc = device_call(call, [&](hipStream_t st) {
        // the three derived constants, each operation rounded once to fp32 (volatile: no contraction, no wider intermediate)
        volatile float omb1 = 1.0f - cfg->beta1, omb2 = 1.0f - cfg->beta2, lr_wd = cfg->lr * cfg->weight_decay;
        volatile float dk = 1.0f - lr_wd;
        const AdamArgs a{W, G, M, V, (float*)S,
                         AdamCfg{cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, cfg->grad_scale, omb1, omb2, dk, cfg->decoupled != 0 ? 1 : 0}, (const uint32_t*)R};
        if (env_switch("SPARTA_ADAM_FUSE")) fused = sgd_fused_image(A);
        live = live_steps_active(A);
        launch_adam_tick(st, a);
        launches = 1;
        if (fused >= 0 && A->dtype == SPARTA_F32) {
            if (live) launch_adam_f32_frag_live(st, A->d_steps[0], A->n_steps[0], a, A->d_a_frag, A->d_A, A->d_live_words);
            else launch_adam_f32_frag(st, A->d_steps[0], A->n_steps[0], a, A->d_a_frag, A->d_A);
            launches++;
        } else if (fused >= 0) {
            const bool bf16 = A->dtype == SPARTA_BF16;
            uint16_t* dst = (uint16_t*)A->d_A.get() + A->upd_base[fused];
            if (live) launch_adam_h16_live(bf16, fused ? 64 : 32, A->kp16, st, A->d_upd_map[fused], A->n_steps[fused], a, dst, A->d_live_words);
            else launch_adam_h16(bf16, fused ? 64 : 32, A->kp16, st, A->d_upd_map[fused], A->n_steps[fused], a, dst);
            launches++;
            if (A->n_t_src > 0) { launch_update_h16_t(bf16, st, A->d_t_src, A->n_t_src, (int)A->w, W, A->d_t_A); launches++; }   // reads the W written above
        } else {
            if (live) launch_adam_blocks_live(st, A->d_prune, A->n_prune, A->d_live_keep, a);
            else launch_adam_step(st, A->nztot, a);
            launches += 1 + launch_images_from(A, st, W);
        }
        a8_requantize(A, st, W);                  // (as in sgd_step_impl)
    });
    if (rc) return rc;
    A->step_last_live = live ? 1 : 0;
    A->step_last_fused = fused >= 0 ? 1 : 0;
    A->step_last_launches = launches;
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_vbs_adam_step(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S, const sparta_adam_cfg* cfg, void* stream,
                                    float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return adam_step_impl("sparta_vbs_adam_step", A, W, G, M, V, S, cfg, nullptr, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_adam_step")
}

extern "C" int sparta_vbs_adam_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S, const sparta_adam_cfg* cfg, const void* R,
                                        void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return adam_step_impl("sparta_vbs_adam_step_ctl", A, W, G, M, V, S, cfg, R, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_adam_step_ctl")
}

// ---- sparta_grad_stats / sparta_grad_ctl_finish (k_gradctl.hip) ---------------------------------------------------------------------------
static_assert(SPARTA_GRAD_CTL_BYTES == kGradCtlBytes && SPARTA_GRAD_STATS_CHUNK == kGradCtlChunk && SPARTA_GRAD_STATS_MAX_GRID == kGradCtlMaxGrid,
              "include/sparta_amd.h and vbs_device.hpp disagree on the control record");

extern "C" int sparta_grad_stats(const float* G, int64_t n, void* R, int32_t accumulate, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (!R) return fail(SPARTA_ERR_INVALID, "sparta_grad_stats: R is NULL");
    if ((uintptr_t)R % 8 != 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_stats: the control record R must be 8-byte aligned");
    if (n < 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_stats: n < 0");
    if (n > 0 && !G) return fail(SPARTA_ERR_INVALID, "sparta_grad_stats: G is NULL with n > 0");
    if ((uintptr_t)G % 4 != 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_stats: G must be 4-byte aligned");
    // handle-free: no guard, and the events of a timed call live for that call
    return device_call(DeviceCall{"sparta_grad_stats", nullptr, (hipStream_t)stream, true, dt_ms, "the reduction"},
                       [&](hipStream_t st) { launch_grad_stats(st, G, n, R, accumulate != 0); });
    SPARTA_GUARD_END("sparta_grad_stats")
}

extern "C" int sparta_grad_ctl_finish(void* R, const sparta_grad_ctl_cfg* cfg, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (!R || !cfg) return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: R or cfg is NULL");
    if ((uintptr_t)R % 8 != 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: the control record R must be 8-byte aligned");
    if (!(cfg->max_norm >= 0.0f)) return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: max_norm must be >= 0 (0: no clipping)");
    if (cfg->growth_interval < 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: growth_interval must be >= 0 (0: the loss scale stays)");
    if (cfg->growth_interval > 0 && (!(cfg->growth_factor >= 1.0f) || !(cfg->backoff_factor > 0.0f && cfg->backoff_factor <= 1.0f)))
        return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: growth_factor must be >= 1 and backoff_factor in (0, 1]");
    for (int i = 0; i < 4; i++)
        if (cfg->reserved[i] != 0) return fail(SPARTA_ERR_INVALID, "sparta_grad_ctl_finish: cfg->reserved must be 0");
    return device_call(DeviceCall{"sparta_grad_ctl_finish", nullptr, (hipStream_t)stream, true},
                       [&](hipStream_t st) { launch_grad_ctl_finish(st, R, cfg->max_norm, cfg->growth_factor, cfg->backoff_factor, cfg->growth_interval); });
    SPARTA_GUARD_END("sparta_grad_ctl_finish")
}

extern "C" int sparta_vbs_step_info(const sparta_vbs_t* A, int64_t* info_out) {
    if (!A || !info_out) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_step_info: NULL argument");
    info_out[0] = A->step_last_fused; info_out[1] = A->step_last_launches; info_out[2] = A->step_last_live; info_out[3] = 0;
    return SPARTA_OK;
}

// ---- block pruning: sparta_vbs_block_table_host, sparta_vbs_block_count, sparta_vbs_block_ssq, sparta_vbs_mask_blocks (k_prune.hip) -------

namespace {

int prune_handle_check(const sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (!A) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!A->from_vbs_arrays)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle was not made from VBS arrays (handles of sparta_vbs_create_from_csr and "
                                            "sparta_vbs_create_transposed do not hold the caller's blocks)");
    return SPARTA_OK;
}

// the device table, made at the first call from the heights and counts kept at creation and the handle's jab, through build_block_table
int ensure_prune_table(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->n_prune >= 0) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload its block table", entry);
    const int64_t nb = A->nblocks;
    if (nb > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": more than 2^31 - 1 blocks");
    std::vector<int32_t> jab32((size_t)nb);
    if (nb > 0) HIP_TRY(hipMemcpy(jab32.data(), A->d_jab, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> jab(jab32.begin(), jab32.end()), table((size_t)nb * 4);
    int64_t n = 0;
    if (int rc = build_block_table(A->cols, A->w, 0, A->block_rows, A->h_row_part.data(), A->h_nzcount.data(), jab.data(), 0, table.data(), &n)) return rc;
    if (n != nb) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the block table disagrees with the handle's block count");
    std::vector<PruneBlock> rec((size_t)nb);
    for (int64_t q = 0; q < nb; q++) {
        if (table[(size_t)(4 * q + 2)] > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": a block of 2^31 or more elements");
        rec[(size_t)q] = PruneBlock{table[(size_t)(4 * q)], (int32_t)table[(size_t)(4 * q + 1)], (int32_t)table[(size_t)(4 * q + 2)]};
    }
    if (nb > 0) HIP_TRY(A->d_prune.upload(rec));
    A->n_prune = nb;
    return SPARTA_OK;
}

// the launches of one entry between the handle's events, behind the block table (built at the first call that has something to do)
template <class Launch>
int prune_call(sparta_vbs_t* A, const char* entry, bool nothing_to_do, void* stream, float* dt_ms, Launch launch) {
    const DeviceCall call{entry, A, (hipStream_t)stream, true, dt_ms, "the kernel", A->ev0, A->ev1, nothing_to_do};
    return open_call(call, [&](hipStream_t) -> int {
        if (!nothing_to_do)
            if (int rc = ensure_prune_table(A, entry)) return rc;
        return timed_launches(call, launch);
    });
}

}  // namespace

extern "C" int sparta_vbs_block_count(const sparta_vbs_t* A, int64_t* n_blocks_out) {
    if (int rc = prune_handle_check(A, "sparta_vbs_block_count")) return rc;
    if (!n_blocks_out) return sparta::fail(SPARTA_ERR_INVALID, "sparta_vbs_block_count: NULL argument");
    *n_blocks_out = A->nblocks;
    return SPARTA_OK;
}

extern "C" int sparta_vbs_block_ssq(sparta_vbs_t* A, const float* W, double* ssq_out, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (int rc = prune_handle_check(A, "sparta_vbs_block_ssq")) return rc;
    if (A->nblocks > 0 && (!ssq_out || (!W && A->nztot > 0))) return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_ssq: W or ssq_out is NULL");
    if ((uintptr_t)W % 4 != 0 || (uintptr_t)ssq_out % 8 != 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_ssq: W must be 4-byte and ssq_out 8-byte aligned");
    return prune_call(A, "sparta_vbs_block_ssq", A->nblocks == 0, stream, dt_ms,
                      [&](hipStream_t st) { launch_block_ssq(st, A->d_prune, A->n_prune, W, ssq_out); });
    SPARTA_GUARD_END("sparta_vbs_block_ssq")
}

extern "C" int sparta_vbs_mask_blocks(sparta_vbs_t* A, const uint8_t* keep, float* T0, float* T1, float* T2, float* T3, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (int rc = prune_handle_check(A, "sparta_vbs_mask_blocks")) return rc;
    if (A->nblocks > 0 && !keep) return fail(SPARTA_ERR_INVALID, "sparta_vbs_mask_blocks: keep is NULL");
    if (((uintptr_t)T0 | (uintptr_t)T1 | (uintptr_t)T2 | (uintptr_t)T3) % 4 != 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_mask_blocks: the tensors must be 4-byte aligned");
    const bool none = !T0 && !T1 && !T2 && !T3;
    return prune_call(A, "sparta_vbs_mask_blocks", A->nblocks == 0 || A->nztot == 0 || none, stream, dt_ms,
                      [&](hipStream_t st) { launch_mask_blocks(st, A->d_prune, A->n_prune, keep, T0, T1, T2, T3); });
    SPARTA_GUARD_END("sparta_vbs_mask_blocks")
}

// ---- repattern: sparta_vbs_repattern_host (the pattern rule, host only), sparta_vbs_move_blocks (k_repattern.hip) -------------------------------------

namespace {

// the block table of a handle on the host ([n_blocks][4], sparta_vbs_block_table_host over the handle's own block-rows), from the heights and counts kept at
// creation and the handle's jab; the handle is not changed
int host_block_table(const sparta_vbs_t* A, const char* entry, std::vector<int64_t>& table) {
    using sparta::fail;
    const int64_t nb = A->nblocks;
    if (nb > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": more than 2^31 - 1 blocks");
    std::vector<int32_t> jab32((size_t)nb);
    if (nb > 0) HIP_TRY(hipMemcpy(jab32.data(), A->d_jab, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> jab(jab32.begin(), jab32.end());
    table.assign((size_t)nb * 4, 0);
    int64_t n = 0;
    if (int rc = build_block_table(A->cols, A->w, 0, A->block_rows, A->h_row_part.data(), A->h_nzcount.data(), jab.data(), 0, table.data(), &n)) return rc;
    if (n != nb) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the block table disagrees with the handle's block count");
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_vbs_move_blocks(sparta_vbs_t* dst, const sparta_vbs_t* src, const int32_t* map, const float* S0, float* D0, const float* S1, float* D1,
                                      const float* S2, float* D2, const float* S3, float* D3, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* me = "sparta_vbs_move_blocks";
    if (int rc = prune_handle_check(dst, me)) return rc;
    if (int rc = prune_handle_check(src, me)) return rc;
    if (dst->device != src->device) return fail(SPARTA_ERR_INVALID, std::string(me) + ": the two handles live on different devices");
    const float* S[4] = {S0, S1, S2, S3};
    float* D[4] = {D0, D1, D2, D3};
    bool any = false;
    for (int q = 0; q < 4; q++) {
        if ((S[q] == nullptr) != (D[q] == nullptr)) return fail(SPARTA_ERR_INVALID, std::string(me) + ": a pair with exactly one NULL pointer");
        if ((uintptr_t)S[q] % 4 != 0 || (uintptr_t)D[q] % 4 != 0) return fail(SPARTA_ERR_INVALID, std::string(me) + ": the tensors must be 4-byte aligned");
        any = any || D[q] != nullptr;
    }
    const int64_t nb = dst->nblocks, nb_src = src->nblocks;
    if (nb > 0 && !map) return fail(SPARTA_ERR_INVALID, std::string(me) + ": map is NULL");
    for (int64_t b = 0; b < nb; b++)
        if (map[b] < -1 || map[b] >= nb_src) return fail(SPARTA_ERR_INVALID, std::string(me) + ": a map entry outside [-1, n_blocks(src))");
    // no D may overlap an S or another D (byte ranges; an empty tensor overlaps nothing)
    const uintptr_t s_bytes = (uintptr_t)src->nztot * 4, d_bytes = (uintptr_t)dst->nztot * 4;
    auto overlap = [](uintptr_t a, uintptr_t an, uintptr_t b, uintptr_t bn) { return an > 0 && bn > 0 && a < b + bn && b < a + an; };
    for (int q = 0; q < 4; q++) {
        if (!D[q]) continue;
        for (int r = 0; r < 4; r++) {
            if (S[r] && overlap((uintptr_t)D[q], d_bytes, (uintptr_t)S[r], s_bytes)) return fail(SPARTA_ERR_INVALID, std::string(me) + ": a destination tensor overlaps a source tensor");
            if (r > q && D[r] && overlap((uintptr_t)D[q], d_bytes, (uintptr_t)D[r], d_bytes)) return fail(SPARTA_ERR_INVALID, std::string(me) + ": two destination tensors overlap");
        }
    }
    const bool nothing_to_do = nb == 0 || dst->nztot == 0 || !any;
    const DeviceCall call{me, dst, (hipStream_t)stream, true, dt_ms, nullptr, dst->ev0, dst->ev1, nothing_to_do};
    return open_call(call, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("build and upload the records of the move (it synchronises)", me);
        std::vector<int64_t> td, ts;
        if (int rc = host_block_table(dst, me, td)) return rc;
        if (int rc = host_block_table(src, me, ts)) return rc;
        std::vector<MoveBlock> rec((size_t)nb);
        for (int64_t b = 0; b < nb; b++) {
            const int64_t n_all = td[(size_t)(4 * b + 2)];
            if (n_all > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(me) + ": a block of 2^31 or more elements");
            const int64_t m = map[b];
            if (m >= 0 && ts[(size_t)(4 * m + 2)] != n_all) return fail(SPARTA_ERR_INVALID, std::string(me) + ": a mapped block differs in size (n_all) from its source block");
            rec[(size_t)b] = MoveBlock{m >= 0 ? ts[(size_t)(4 * m)] : 0, td[(size_t)(4 * b)], (int32_t)n_all, m >= 0 ? 1 : 0};
        }
        if (!nothing_to_do) {
            HIP_TRY(hipStreamSynchronize(st));                                // (the kernel of an earlier call may still read the records)
            if (int rc = dst->d_repat.ensure(rec.size() * sizeof(MoveBlock), dst->retired)) return rc;
            HIP_TRY(hipMemcpy(dst->d_repat, rec.data(), rec.size() * sizeof(MoveBlock), hipMemcpyHostToDevice));
        }
        return timed_launches(call, [&](hipStream_t) { launch_move_blocks(st, (const MoveBlock*)dst->d_repat, nb, S, D); });
    });
    SPARTA_GUARD_END("sparta_vbs_move_blocks")
}

// ---- dense <-> blocks: sparta_dense_block_ssq, sparta_vbs_gather_dense, sparta_vbs_scatter_dense (k_dense.hip) ---------------------------------------
namespace {

// what the three entries ask of D; D == NULL is judged by the caller (it depends on whether there is work)
int dense_operand_check(const char* entry, const void* D, int64_t ldd, int32_t layout, int32_t dtype, int64_t rows, int64_t cols) {
    using sparta::fail;
    const std::string e(entry);
    if (layout != SPARTA_ROW_MAJOR && layout != SPARTA_COL_MAJOR) return fail(SPARTA_ERR_INVALID, e + ": unknown layout " + std::to_string(layout) + " of D");
    if (dtype != SPARTA_F32 && dtype != SPARTA_F16 && dtype != SPARTA_BF16) return fail(SPARTA_ERR_INVALID, e + ": unknown dtype " + std::to_string(dtype) + " of D");
    if (ldd < (layout == SPARTA_ROW_MAJOR ? cols : rows))
        return fail(SPARTA_ERR_INVALID, e + ": the leading dimension of D is too small (row-major: ldd >= cols, column-major: ldd >= rows)");
    if ((uintptr_t)D % (dtype == SPARTA_F32 ? 4u : 2u) != 0) return fail(SPARTA_ERR_INVALID, e + ": D is not aligned to its element size");
    if (rows > INT32_MAX || cols > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, e + ": 2^31 or more rows or columns");
    return SPARTA_OK;
}

// the chunk records, made at the first call from the block table of the handle (build_block_table over the heights and counts kept at creation and the
// handle's jab): per stored block of height > 0 one record per kDenseChunk rows
int ensure_dense_table(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->n_dense >= 0) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload its table of block chunks", entry);
    std::vector<int64_t> table;
    if (int rc = host_block_table(A, entry, table)) return rc;
    const int64_t nb = A->nblocks, w = A->w;
    std::vector<DenseItem> items;
    std::vector<int64_t> words((size_t)nb);                               // (block-row << 32 | block column: equal neighbours once sorted = a column stored twice)
    for (int64_t q = 0; q < nb; q++) words[(size_t)q] = table[(size_t)(4 * q + 3)];
    std::sort(words.begin(), words.end());
    const bool dup = std::adjacent_find(words.begin(), words.end()) != words.end();
    for (int64_t q = 0; q < nb; q++) {
        const int64_t* t = table.data() + 4 * q;
        const int64_t ib = t[3] >> 32, jb = t[3] & 0xffffffffll;
        if (t[2] > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": a block of 2^31 or more elements");
        const int64_t r0 = A->h_row_part[(size_t)ib], h = A->h_row_part[(size_t)ib + 1] - r0, c0 = jb * w;
        for (int64_t i0 = 0; i0 < h; i0 += kDenseChunk)
            items.push_back(DenseItem{t[0], (int32_t)r0, (int32_t)c0, (int32_t)h, (int32_t)i0, (int32_t)std::min<int64_t>(kDenseChunk, h - i0),
                                      (int32_t)std::min(w, A->cols - c0)});
    }
    if ((int64_t)items.size() > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": more than 2^31 - 1 block chunks");
    if (!items.empty()) HIP_TRY(A->d_dense.upload(items));
    A->dense_dup = dup;
    A->n_dense = (int64_t)items.size();
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_dense_block_ssq(const void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, int64_t rows, int64_t cols, int64_t block_rows, int64_t block_col_size,
                                      const int64_t* row_part, double* ssq_out, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* me = "sparta_dense_block_ssq";
    if (rows < 0 || cols < 0 || block_rows < 0 || block_col_size <= 0) return fail(SPARTA_ERR_INVALID, std::string(me) + ": bad dimensions");
    if (int rc = dense_operand_check(me, D, ldd, d_layout, d_dtype, rows, cols)) return rc;
    if (block_rows > 0 && !row_part) return fail(SPARTA_ERR_INVALID, std::string(me) + ": row_part is NULL with block_rows > 0");
    if ((uintptr_t)row_part % 8 != 0 || (uintptr_t)ssq_out % 8 != 0) return fail(SPARTA_ERR_INVALID, std::string(me) + ": row_part and ssq_out must be 8-byte aligned");
    const int64_t block_cols = cols > 0 ? (cols - 1) / block_col_size + 1 : 0;
    if (block_cols > 0 && block_rows > INT32_MAX / block_cols) return fail(SPARTA_ERR_UNSUPPORTED, std::string(me) + ": more than 2^31 - 1 grid blocks");
    const bool nothing = block_rows == 0 || block_cols == 0;
    if (!nothing && !ssq_out) return fail(SPARTA_ERR_INVALID, std::string(me) + ": ssq_out is NULL");
    if (!nothing && rows > 0 && !D) return fail(SPARTA_ERR_INVALID, std::string(me) + ": D is NULL");
    return device_call(DeviceCall{me, nullptr, (hipStream_t)stream, true, dt_ms, "the kernel", nullptr, nullptr, nothing}, [&](hipStream_t st) {
        launch_dense_block_ssq(st, D, ldd, d_layout == SPARTA_ROW_MAJOR, d_dtype, rows, cols, block_rows, block_col_size, row_part, ssq_out);
    });
    SPARTA_GUARD_END("sparta_dense_block_ssq")
}

extern "C" int sparta_vbs_gather_dense(sparta_vbs_t* A, const void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, float* T, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* me = "sparta_vbs_gather_dense";
    if (int rc = prune_handle_check(A, me)) return rc;
    if (int rc = dense_operand_check(me, D, ldd, d_layout, d_dtype, A->rows, A->cols)) return rc;
    if ((uintptr_t)T % 4 != 0) return fail(SPARTA_ERR_INVALID, std::string(me) + ": T must be 4-byte aligned");
    const bool nothing = A->nztot == 0;
    if (!nothing && (!D || !T)) return fail(SPARTA_ERR_INVALID, std::string(me) + ": D or T is NULL");
    const DeviceCall call{me, A, (hipStream_t)stream, true, dt_ms, "the kernel", A->ev0, A->ev1, nothing};
    return open_call(call, [&](hipStream_t) -> int {
        if (!nothing)
            if (int rc = ensure_dense_table(A, me)) return rc;
        return timed_launches(call, [&](hipStream_t st) {
            launch_dense_gather(st, A->d_dense, A->n_dense, D, ldd, d_layout == SPARTA_ROW_MAJOR, d_dtype, (int)A->w, T);
        });
    });
    SPARTA_GUARD_END("sparta_vbs_gather_dense")
}

extern "C" int sparta_vbs_scatter_dense(sparta_vbs_t* A, const float* T, void* D, int64_t ldd, int32_t d_layout, int32_t d_dtype, int32_t fill, void* stream,
                                        float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* me = "sparta_vbs_scatter_dense";
    if (int rc = prune_handle_check(A, me)) return rc;
    if (int rc = dense_operand_check(me, D, ldd, d_layout, d_dtype, A->rows, A->cols)) return rc;
    if ((uintptr_t)T % 4 != 0) return fail(SPARTA_ERR_INVALID, std::string(me) + ": T must be 4-byte aligned");
    const bool blocks = A->nztot > 0, region = fill != 0 && A->rows > 0 && A->cols > 0, nothing = !blocks && !region;
    if (!nothing && !D) return fail(SPARTA_ERR_INVALID, std::string(me) + ": D is NULL");
    if (blocks && !T) return fail(SPARTA_ERR_INVALID, std::string(me) + ": T is NULL");
    const bool row_major = d_layout == SPARTA_ROW_MAJOR;
    if (region) {
        const int64_t esz = d_dtype == SPARTA_F32 ? 4 : 2, segs = dense_fill_segs((row_major ? A->cols : A->rows) * esz), n_runs = row_major ? A->rows : A->cols;
        if (n_runs > INT32_MAX / segs) return fail(SPARTA_ERR_UNSUPPORTED, std::string(me) + ": the fill needs more than 2^31 - 1 workgroups");
    }
    const DeviceCall call{me, A, (hipStream_t)stream, true, dt_ms, "the kernels", A->ev0, A->ev1, nothing};
    return open_call(call, [&](hipStream_t) -> int {
        if (blocks) {
            if (int rc = ensure_dense_table(A, me)) return rc;
            if (A->dense_dup)
                return fail(SPARTA_ERR_UNSUPPORTED, std::string(me) + ": a block-row of the handle stores a block column twice (two blocks would write the same elements of D)");
        }
        return timed_launches(call, [&](hipStream_t st) {
            if (region) launch_dense_fill(st, D, ldd, row_major, d_dtype, A->rows, A->cols);
            if (blocks) launch_dense_scatter(st, A->d_dense, A->n_dense, T, D, ldd, row_major, d_dtype);
        });
    });
    SPARTA_GUARD_END("sparta_vbs_scatter_dense")
}

// ---- the live-block set: sparta_vbs_set_live_blocks, _live_info, _live_lists_get, _live_lists_host (k_live.hip) ----------------------------------
namespace {

// the pattern-only helper arrays, made at the first sparta_vbs_set_live_blocks from what the handle keeps (heights, counts, jab; the block table for the zeros
// of sddmm), and the arrays the launches of every call fill
int ensure_live_arrays(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->live_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload the helper arrays of the live set", entry);
    if (int rc = ensure_prune_table(A, entry)) return rc;
    const int64_t nb = A->nblocks;
    std::vector<int32_t> jab32((size_t)nb);
    if (nb > 0) HIP_TRY(hipMemcpy(jab32.data(), A->d_jab, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    const std::vector<int64_t> jab(jab32.begin(), jab32.end());
    LiveMapsHost M;
    if (int rc = build_live_maps(A->cols, A->w, 0, A->block_rows, A->h_row_part.data(), A->h_nzcount.data(), jab.data(), 0, M)) return rc;
    std::vector<int32_t> goff;
    for (int64_t ib = 0; ib < A->block_rows; ib++)
        if (A->h_row_part[(size_t)ib + 1] > A->h_row_part[(size_t)ib]) goff.push_back((int32_t)M.goff[(size_t)ib]);
    if ((int64_t)goff.size() != A->n_brows || M.first_block.back() != nb) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the live-set maps disagree with the handle's block-rows");
    A->live_n_groups = M.goff.back();
    HIP_TRY(A->d_live_keep.alloc((size_t)nb, 16));
    HIP_TRY(A->d_live_goff.alloc(goff.size(), 16));
    HIP_TRY(A->d_live_groups.alloc((size_t)A->live_n_groups, 16));
    HIP_TRY(A->d_live_gcount.alloc(goff.size(), 16));
    if (!goff.empty()) HIP_TRY(hipMemcpy(A->d_live_goff, goff.data(), goff.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    A->live_n_tlist = 0;
    A->live_block_cols = (int64_t)M.tptr.size() - 1;
    if (A->create_flags & SPARTA_CREATE_TRANSPOSE) {
        const int64_t panels = (A->w + 31) / 32;
        if (A->live_block_cols * panels != A->n_t_items || (int64_t)M.tmap.size() != A->n_t_blocks)
            return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the live-set maps disagree with the handle's block-column index");
        A->live_n_tlist = (int64_t)M.tmap.size();
        HIP_TRY(A->d_live_tmap.alloc(M.tmap.size(), 16));
        HIP_TRY(A->d_live_tids.alloc(M.tmap.size(), 16));
        HIP_TRY(A->d_live_t_blocks.alloc(M.tmap.size(), 16));
        HIP_TRY(A->d_live_tcount.alloc((size_t)A->live_block_cols, 16));
        HIP_TRY(A->d_live_t_items.alloc((size_t)A->n_t_items, 16));
        if (!M.tmap.empty()) HIP_TRY(hipMemcpy(A->d_live_tmap, M.tmap.data(), M.tmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    A->live_built = true;
    return SPARTA_OK;
}

// the pattern-only map of the live words (handles with a fused image only): word -> block number, from the block table and the plan's own records of where
// a step / a slice half starts in mab.  Built once, at the first enabling sparta_vbs_set_live_steps or sparta_vbs_set_live_forward: both read the same words.
int ensure_live_word_map(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->live_words_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload the map of the live words", entry);
    if (int rc = ensure_live_arrays(A, entry)) return rc;
    const int ty = sgd_fused_image(A);
    if (ty >= 0 && A->nztot > 0) {
        const int64_t nb = A->n_prune;
        std::vector<PruneBlock> tab((size_t)nb);
        if (nb > 0) HIP_TRY(hipMemcpy(tab.data(), A->d_prune, (size_t)nb * sizeof(PruneBlock), hipMemcpyDeviceToHost));
        std::vector<int64_t> off((size_t)nb);
        for (int64_t b = 0; b < nb; b++) off[(size_t)b] = tab[(size_t)b].off;
        std::vector<int64_t> first;
        std::vector<int32_t> ld;
        int64_t span = SK_KP;
        if (A->dtype == SPARTA_F32) {                       // one word per step: its 32 columns start at a_off, h apart
            for (int64_t q = 0; q < A->n_steps[0]; q++) { first.push_back(A->h_steps[0][(size_t)q].a_off); ld.push_back(A->h_steps[0][(size_t)q].h); }
        } else {                                            // two words per slice: the kp columns of its rows 0..31 and of its rows 32..63 -- the upper and the
                                                            // lower block-row of a pair tile (rows_lo = 32 or 0), the one block of an ordinary tile (rows_hi = 0)
            std::vector<UpdSlice> map((size_t)A->n_steps[ty]);
            HIP_TRY(hipMemcpy(map.data(), A->d_upd_map[ty], map.size() * sizeof(UpdSlice), hipMemcpyDeviceToHost));
            span = A->kp16;
            for (const UpdSlice& u : map) {
                first.push_back(u.rows_lo > 0 ? u.off_lo : -1); ld.push_back(u.h_lo);
                if (u.rows_hi > 0) { first.push_back(u.off_hi); ld.push_back(u.h_hi); }
                else { first.push_back(u.rows_lo > 32 ? u.off_lo : -1); ld.push_back(u.h_lo); }
            }
        }
        std::vector<int32_t> wmap(first.size());
        if (int rc = build_live_word_map(off.data(), nb, A->nztot, first.data(), ld.data(), (int64_t)first.size(), span, wmap.data())) return rc;
        A->live_n_words = (int64_t)wmap.size();
        HIP_TRY(A->d_live_wmap.alloc(wmap.size(), 16));
        HIP_TRY(A->d_live_words.alloc(wmap.size(), 16));
        if (!wmap.empty()) HIP_TRY(hipMemcpy(A->d_live_wmap, wmap.data(), wmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    A->live_words_built = true;
    return SPARTA_OK;
}

int ensure_live_step_arrays(sparta_vbs_t* A, const char* entry) {
    if (A->live_steps_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload the helper arrays of the live steps", entry);
    if (int rc = ensure_live_word_map(A, entry)) return rc;
    A->live_steps_built = true;
    return SPARTA_OK;
}

// Live forward: which stream image of the handle has live sibling kernels -- a 16-bit handle whose one stream image holds every stored element (the handles
// the word map covers two words per step: no hub plan, one image, block width a multiple of 32).  -1: the plain kernels run under the switch.
int live_forward_image(const sparta_vbs_t* A) {
    if (A->dtype == SPARTA_F32 || A->nztot <= 0 || !(A->create_flags & SPARTA_CREATE_UPDATABLE)) return -1;
    return sgd_fused_image(A);
}

// the second record array (a copy of the plain one, padding included: what lies outside the ranges is never rewritten), the second range array and the
// segment map of that image.  Built once, at the first enabling sparta_vbs_set_live_forward.
int ensure_live_forward_arrays(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->live_fwd_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload the helper arrays of the live forward product", entry);
    if (int rc = ensure_live_word_map(A, entry)) return rc;
    const int ty = live_forward_image(A);
    if (ty >= 0 && A->live_n_words == 2 * A->n_steps[ty]) {
        const std::vector<StepRec>& hs = A->h_steps[ty];
        const int64_t n = A->n_steps[ty], n_ranges = (int64_t)A->n_workers * ((ty == 0 && A->wide16) ? 2 : 1);
        if ((int64_t)hs.size() < n) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the handle keeps no host copy of its step records");
        std::vector<int32_t> ranges((size_t)n_ranges * 2);
        HIP_TRY(hipMemcpy(ranges.data(), A->d_wrange[ty], ranges.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < n_ranges; r++)
            if (ranges[(size_t)(2 * r)] < 0 || ranges[(size_t)(2 * r + 1)] > n)
                return fail(SPARTA_ERR_INVALID, std::string(entry) + ": a worker range of the plan lies outside its step records");
        std::vector<int32_t> seg_last((size_t)n);
        live_forward_segments(hs.data(), n, ranges.data(), n_ranges, seg_last.data());
        HIP_TRY(A->d_fwd_steps.upload(hs));
        HIP_TRY(A->d_fwd_wrange.upload(ranges));
        HIP_TRY(A->d_fwd_seg_last.alloc(seg_last.size(), 16));
        HIP_TRY(hipMemcpy(A->d_fwd_seg_last, seg_last.data(), seg_last.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        A->fwd_n_ranges = n_ranges; A->fwd_n_alloc = (int64_t)hs.size();
        A->live_fwd_ty = ty;
    }
    A->live_fwd_built = true;
    return SPARTA_OK;
}

// the compacted records and live ranges behind the words of the current snapshot, in stream order
void launch_live_forward_lists(sparta_vbs_t* A, hipStream_t st) {
    const int ty = A->live_fwd_ty;
    if (!A->live_fwd_built || ty < 0) return;
    launch_live_forward_compact(st, A->d_steps[ty], A->d_fwd_seg_last, A->d_wrange[ty], A->fwd_n_ranges, A->d_live_words, ty == 1, A->d_fwd_steps, A->d_fwd_wrange);
}

}  // namespace

extern "C" int sparta_vbs_set_live_steps(sparta_vbs_t* A, int32_t enable, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_set_live_steps";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!(A->create_flags & SPARTA_CREATE_UPDATABLE))
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle was not made with SPARTA_CREATE_UPDATABLE (it takes no steps)");
    if (!enable) {                               // host state only
        A->live_steps = false;
        return SPARTA_OK;
    }
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (int rc = ensure_live_step_arrays(A, entry)) return rc;
        if (A->live_on && A->live_n_words > 0) {     // a set is installed already: the words follow from its snapshot
            launch_live_step_words(st, A->d_live_wmap, A->live_n_words, A->d_live_keep, A->d_live_words);
            HIP_TRY(hipGetLastError());
        }
        A->live_steps = true;
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_set_live_steps")
}

extern "C" int sparta_vbs_set_live_blocks(sparta_vbs_t* A, const uint8_t* keep, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_set_live_blocks";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!keep) {                                 // host state only: the products launch what they launched before a live set was installed
        A->live_on = false;
        return SPARTA_OK;
    }
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (int rc = ensure_live_arrays(A, entry)) return rc;
        launch_live_sddmm(st, A->d_brows, A->n_brows, (int)A->w, keep, A->nblocks, A->d_live_keep, A->d_live_goff, A->d_live_groups, A->d_live_gcount);
        if (A->create_flags & SPARTA_CREATE_TRANSPOSE)
            launch_live_spmm_t(st, A->d_t_items, A->d_t_blocks, A->d_live_tmap, A->live_block_cols, (int)((A->w + 31) / 32), keep, A->d_live_t_items, A->d_live_t_blocks,
                               A->d_live_tids, A->d_live_tcount);
        // live steps: the words of the image kernel behind the snapshot, in stream order (written whether or not the switch is on right now, once they exist)
        if (A->live_words_built && A->live_n_words > 0) launch_live_step_words(st, A->d_live_wmap, A->live_n_words, A->d_live_keep, A->d_live_words);
        // live forward: the compacted records of the stream image behind the words (likewise written once they exist, whatever the switch says right now)
        launch_live_forward_lists(A, st);
        // the fp8 image with a live-block set: the compaction rewrote every position from the plain records, the exponent words go back in behind it
        a8_live_place_scales(A, st);
        HIP_TRY(hipGetLastError());
        A->live_on = true;
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_set_live_blocks")
}

// ---- sparta_vbs_sddmm_block_ssq: the score form of the SDDMM (k_sddmm.hip) -----------------------------------------------------------------------
namespace {

// the pattern-only helpers (the live set's goff, made without installing a set; the slot offset of every block-row; the finish record of every block) and the
// arrays every call writes: the snapshot of sel, its group lists and counts, the slots
int ensure_score_arrays(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->score_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("build and upload the helper arrays of the block scores", entry);
    if (int rc = ensure_sddmm_items(A)) return rc;
    if (int rc = ensure_live_arrays(A, entry)) return rc;
    const int64_t nb = A->nblocks, w = A->w;
    std::vector<int64_t> soff;
    std::vector<ScoreBlock> rec((size_t)nb);
    int64_t slots = 0, q = 0;
    for (int64_t ib = 0; ib < A->block_rows; ib++) {
        const int64_t h = A->h_row_part[(size_t)ib + 1] - A->h_row_part[(size_t)ib], tiles = (h + 31) / 32, nq = A->h_nzcount[(size_t)ib] * w;
        if (h > 0) soff.push_back(slots);
        for (int64_t b = 0; b < A->h_nzcount[(size_t)ib]; b++, q++) rec[(size_t)q] = ScoreBlock{slots + b * w, nq, (int32_t)tiles, 0};
        slots += tiles * nq;
    }
    if ((int64_t)soff.size() != A->n_brows || q != nb) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the score maps disagree with the handle's block-rows");
    HIP_TRY(A->d_score_keep.alloc((size_t)nb, 16));
    HIP_TRY(A->d_score_ones.alloc((size_t)nb, 16));
    HIP_TRY(A->d_score_groups.alloc((size_t)A->live_n_groups, 16));
    HIP_TRY(A->d_score_gcount.alloc(soff.size(), 16));
    HIP_TRY(A->d_score_soff.alloc(soff.size(), 16));
    HIP_TRY(A->d_score_blocks.alloc(rec.size(), 16));
    HIP_TRY(A->d_score_slots.alloc((size_t)slots, 16));
    if (nb > 0) {
        HIP_TRY(hipMemset(A->d_score_ones, 1, (size_t)nb));
        HIP_TRY(hipMemcpy(A->d_score_blocks, rec.data(), rec.size() * sizeof(ScoreBlock), hipMemcpyHostToDevice));
    }
    if (!soff.empty()) HIP_TRY(hipMemcpy(A->d_score_soff, soff.data(), soff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    A->score_built = true;
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_vbs_sddmm_block_ssq(sparta_vbs_t* A, const void* X, int64_t ldx, const void* Y, int64_t ldy, int32_t k, const uint8_t* sel, double* ssq_out,
                                          void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_sddmm_block_ssq";
    if (k <= 0) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": k must be > 0");
    if (!A) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (A->ext_sparse)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle does not hold the dense blocks of every block-row (made by sparta_vbs_create_from_csr)");
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (A->nblocks > 0 && (!X || !Y || !ssq_out)) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": X, Y or ssq_out is NULL");
    if ((uintptr_t)ssq_out % 8 != 0) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": ssq_out must be 8-byte aligned");
    if (ldx < A->rows || ldy < A->cols) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": ldx < rows or ldy < cols");
    if (ldx > (INT64_C(1) << 61) / k || ldy > (INT64_C(1) << 61) / k) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": ldx * k or ldy * k beyond 2^61");
    if (A->dtype != SPARTA_F32 && ((ldx | ldy) & 1)) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": 16-bit handles need even ldx, ldy");
    if (A->nblocks == 0) return SPARTA_OK;

    const DeviceCall call{entry, A, (hipStream_t)stream, true, dt_ms, "the product", A->ev0, A->ev1};
    return open_call(call, [&](hipStream_t st) -> int {
        if (int rc = ensure_score_arrays(A, entry)) return rc;

        SddmmParams p;
        p.brows = A->d_brows; p.jab = A->d_jab; p.items = A->d_sd_items;
        p.X = X; p.Y = Y; p.G = nullptr;
        p.ldx = ldx; p.ldy = ldy; p.cols = A->cols;
        p.k = k; p.w = (int32_t)A->w; p.accumulate = 0; p.pad = 0;
        return timed_launches(call, [&](hipStream_t) {
            // the lists of sel, by the kernel of the live set into the score call's own arrays: the live set of the handle, installed or not, is neither read nor written
            launch_live_sddmm(st, A->d_brows, A->n_brows, (int)A->w, sel ? sel : A->d_score_ones, A->nblocks, A->d_score_keep, A->d_live_goff, A->d_score_groups,
                              A->d_score_gcount);
            launch_sddmm_score(A->dtype, (unsigned)A->n_sd_items, st, p, SddmmLive{A->d_score_groups, A->d_live_goff, A->d_score_gcount, A->d_score_keep},
                               SddmmScore{A->d_score_slots, A->d_score_soff});
            launch_sddmm_score_finish(st, A->d_score_blocks, A->nblocks, (int)A->w, A->d_score_keep, A->d_score_slots, ssq_out);
        });
    });
    SPARTA_GUARD_END("sparta_vbs_sddmm_block_ssq")
}

extern "C" int sparta_vbs_set_live_forward(sparta_vbs_t* A, int32_t enable, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_set_live_forward";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!(A->create_flags & SPARTA_CREATE_UPDATABLE))
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle was not made with SPARTA_CREATE_UPDATABLE (it keeps no map from its steps to its blocks)");
    if (!enable) {                               // host state only
        A->live_fwd = false;
        return SPARTA_OK;
    }
    if (A->a8_on)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the fp8 weight image is on (sparta_vbs_set_forward_a8) and the two do not combine -- switch it off first");
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (int rc = ensure_live_forward_arrays(A, entry)) return rc;
        if (A->live_on && A->live_fwd_ty >= 0) {     // a set is installed already: words and lists follow from its snapshot
            launch_live_step_words(st, A->d_live_wmap, A->live_n_words, A->d_live_keep, A->d_live_words);
            launch_live_forward_lists(A, st);
            HIP_TRY(hipGetLastError());
        }
        A->live_fwd = true;
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_set_live_forward")
}

extern "C" int sparta_vbs_live_forward_info(sparta_vbs_t* A, int64_t* info_out, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_live_forward_info";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!info_out) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL argument");
    std::memset(info_out, 0, 8 * sizeof(int64_t));
    const int ty = A->live_fwd_built ? A->live_fwd_ty : live_forward_image(A);
    info_out[0] = A->live_fwd ? 1 : 0;
    info_out[1] = ty + 1;
    info_out[2] = A->fwd_last_form[0];
    info_out[3] = A->fwd_last_form[1];
    info_out[4] = ty >= 0 ? A->n_steps[ty] : 0;
    info_out[6] = A->n_split;
    info_out[7] = A->live_fwd_built && ty >= 0 ? A->fwd_n_ranges : 0;
    if (!A->live_on || !A->live_fwd_built || ty < 0) return SPARTA_OK;
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("read the live ranges back (synchronises)", entry);
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<int32_t> ranges((size_t)A->fwd_n_ranges * 2);
        if (!ranges.empty()) HIP_TRY(hipMemcpy(ranges.data(), A->d_fwd_wrange, ranges.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < A->fwd_n_ranges; r++) info_out[5] += std::max(0, ranges[(size_t)(2 * r + 1)] - ranges[(size_t)(2 * r)]);
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_live_forward_info")
}

extern "C" int sparta_vbs_live_forward_lists_get(sparta_vbs_t* A, void* steps_plain, int32_t* ranges_plain, uint8_t* live_bits, void* steps_live, int32_t* ranges_live,
                                                 void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_live_forward_lists_get";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!A->live_on) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": no live set is installed");
    if (!A->live_fwd_built || A->live_fwd_ty < 0) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle has no live forward lists");
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("read the live forward lists back (synchronises)", entry);
        HIP_TRY(hipStreamSynchronize(st));
        const int ty = A->live_fwd_ty;
        const size_t n = (size_t)A->n_steps[ty], nr = (size_t)A->fwd_n_ranges;
        if (steps_plain && n > 0) HIP_TRY(hipMemcpy(steps_plain, A->d_steps[ty], n * sizeof(StepRec), hipMemcpyDeviceToHost));
        if (steps_live && n > 0) HIP_TRY(hipMemcpy(steps_live, A->d_fwd_steps, n * sizeof(StepRec), hipMemcpyDeviceToHost));
        if (ranges_plain && nr > 0) HIP_TRY(hipMemcpy(ranges_plain, A->d_wrange[ty], nr * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ranges_live && nr > 0) HIP_TRY(hipMemcpy(ranges_live, A->d_fwd_wrange, nr * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (live_bits && n > 0) {
            std::vector<uint32_t> words(2 * n);
            HIP_TRY(hipMemcpy(words.data(), A->d_live_words, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < words.size(); i++) live_bits[i] = words[i] != 0u ? 1 : 0;
        }
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_live_forward_lists_get")
}

// ---- sparta_vbs_set_forward_a8: the fp8 (e4m3) weight image of a 16-bit handle (k_h16_a8.hip) ---------------------------------------------------
namespace {

// the image and the private records: a 16-bit updatable handle whose one stream image holds every stored element exactly once (what live forward asks), with
// slice s of the image behind step s of the records (the quantise kernel writes the exponents of slice s into record s)
int ensure_a8_arrays(sparta_vbs_t* A, const char* entry) {
    using sparta::fail;
    if (A->a8_built) return SPARTA_OK;
    if (g_capturing) return capture_refusal("allocate the fp8 image", entry);
    const int ty = live_forward_image(A);
    if (ty < 0)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": needs a 16-bit handle made with SPARTA_CREATE_UPDATABLE whose one stream image holds every stored "
                                                                 "element (no hub plan, no second image, a block width that is a multiple of 32)");
    const std::vector<StepRec>& hs = A->h_steps[ty];
    const int64_t n = A->n_steps[ty], slice = (int64_t)(ty ? 64 : 32) * A->kp16;
    if ((int64_t)hs.size() < n) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the handle keeps no host copy of its step records");
    for (int64_t q = 0; q < n; q++)
        if (hs[(size_t)q].a_off != A->upd_base[ty] + q * slice)
            return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the slices of the stream image are not in step order");
    A->a8_bytes = A->a_bytes / (int64_t)sizeof(uint16_t);      // one byte per element of the 16-bit image, its padding included
    HIP_TRY(A->d_a8.alloc((size_t)A->a8_bytes));
    HIP_TRY(hipMemset(A->d_a8, 0, (size_t)A->a8_bytes));
    HIP_TRY(A->d_a8_steps.upload(hs));
    A->a8_n_groups = n * (ty ? 2 : 1);
    A->a8_ty = ty;
    A->a8_built = true;
    return SPARTA_OK;
}

}  // namespace

extern "C" int sparta_vbs_set_forward_a8(sparta_vbs_t* A, int32_t enable, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_set_forward_a8";
    if (!A) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!enable) {                               // host state only; the image goes stale from here on (and sparta_vbs_set_a8_live, which needs it, goes off)
        A->a8_on = false;
        A->a8_valid = false;
        A->a8_live = false;
        return SPARTA_OK;
    }
    if (A->ext_sparse || A->dtype == SPARTA_F32 || !(A->create_flags & SPARTA_CREATE_UPDATABLE))
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": needs a 16-bit handle made with SPARTA_CREATE_UPDATABLE (sparta_vbs_create_range_ex)");
    if (A->live_fwd)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": live forward is on (sparta_vbs_set_live_forward) and the two do not combine -- switch it off first");
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (int rc = ensure_a8_arrays(A, entry)) return rc;
        if (!A->a8_on) A->a8_valid = false;          // invalid until the next write of values
        A->a8_on = true;
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_set_forward_a8")
}

extern "C" int sparta_vbs_a8_info(sparta_vbs_t* A, int64_t* info_out, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_a8_info";
    if (!A || !info_out) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL argument");
    std::memset(info_out, 0, 8 * sizeof(int64_t));
    const int ty = A->a8_built ? A->a8_ty : ((A->ext_sparse || A->dtype == SPARTA_F32) ? -1 : live_forward_image(A));
    info_out[0] = A->a8_on ? 1 : 0;
    info_out[1] = A->a8_on && A->a8_valid ? 1 : 0;
    info_out[2] = ty + 1;
    info_out[3] = A->fwd_last_form[0];
    info_out[4] = A->fwd_last_form[1];
    info_out[5] = ty >= 0 ? A->n_steps[ty] * (ty ? 2 : 1) : 0;
    info_out[6] = A->a8_bytes;
    info_out[7] = A->a8_launches;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_a8_info")
}

// ---- sparta_vbs_set_a8_live: the product on the fp8 image skips dead blocks (k_h16_a8_live.hip) -------------------------------------------------
extern "C" int sparta_vbs_set_a8_live(sparta_vbs_t* A, int32_t enable, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_set_a8_live";
    if (!A) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!enable) {                               // host state only
        A->a8_live = false;
        return SPARTA_OK;
    }
    if (!A->a8_on || !A->a8_built || A->a8_ty < 0)
        return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the fp8 weight image is off -- switch it on first (sparta_vbs_set_forward_a8)");
    if (int rc = prune_handle_check(A, entry)) return rc;
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (int rc = ensure_live_forward_arrays(A, entry)) return rc;      // the word map, seg_last and the compacted arrays of live forward: the same ones
        if (A->live_fwd_ty != A->a8_ty)
            return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the stream image that has the fp8 image has no live forward lists");
        A->a8_live = true;
        if (A->live_on) {                            // a set is installed already: words, lists and scales follow from its snapshot
            launch_live_step_words(st, A->d_live_wmap, A->live_n_words, A->d_live_keep, A->d_live_words);
            launch_live_forward_lists(A, st);
            a8_live_place_scales(A, st);
            HIP_TRY(hipGetLastError());
        }
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_set_a8_live")
}

extern "C" int sparta_vbs_a8_live_info(sparta_vbs_t* A, int64_t* info_out, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_a8_live_info";
    if (!A || !info_out) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL argument");
    std::memset(info_out, 0, 8 * sizeof(int64_t));
    const int ty = A->a8_built ? A->a8_ty : ((A->ext_sparse || A->dtype == SPARTA_F32) ? -1 : live_forward_image(A));
    const bool lists = A->live_fwd_built && ty >= 0 && A->live_fwd_ty == ty;
    info_out[0] = A->a8_live ? 1 : 0;
    info_out[1] = A->a8_live && A->a8_on && A->a8_valid && A->a8_built && A->live_on && lists ? 1 : 0;
    info_out[2] = ty + 1;
    info_out[3] = ty >= 0 ? A->n_steps[ty] : 0;
    info_out[5] = A->a8_live_launches;
    if (!A->live_on || !lists) return SPARTA_OK;
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("read the live ranges back (synchronises)", entry);
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<int32_t> ranges((size_t)A->fwd_n_ranges * 2);
        if (!ranges.empty()) HIP_TRY(hipMemcpy(ranges.data(), A->d_fwd_wrange, ranges.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < A->fwd_n_ranges; r++) info_out[4] += std::max(0, ranges[(size_t)(2 * r + 1)] - ranges[(size_t)(2 * r)]);
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_a8_live_info")
}

extern "C" int sparta_vbs_a8_get(sparta_vbs_t* A, uint8_t* codes, int32_t* exps, int32_t* group, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_a8_get";
    if (!A) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!A->a8_built || A->a8_ty < 0) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the handle has no fp8 image (sparta_vbs_set_forward_a8 was never on)");
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("read the fp8 image back (synchronises)", entry);
        HIP_TRY(hipStreamSynchronize(st));
        const int ty = A->a8_ty, tms = ty ? 64 : 32, kp = A->kp16;
        const int64_t n = A->n_steps[ty], slice = (int64_t)tms * kp;
        std::vector<UpdSlice> map((size_t)n);
        std::vector<StepRec> recs((size_t)n);
        std::vector<uint8_t> img((size_t)(n * slice));
        if (n > 0) {
            HIP_TRY(hipMemcpy(map.data(), A->d_upd_map[ty], map.size() * sizeof(UpdSlice), hipMemcpyDeviceToHost));
            if (exps) HIP_TRY(hipMemcpy(recs.data(), A->d_a8_steps, recs.size() * sizeof(StepRec), hipMemcpyDeviceToHost));
            if (codes) HIP_TRY(hipMemcpy(img.data(), A->d_a8 + A->upd_base[ty], img.size(), hipMemcpyDeviceToHost));
        }
        for (int64_t s = 0; s < n; s++) {
            const UpdSlice& u = map[(size_t)s];
            const uint32_t word = (uint32_t)recs[(size_t)s].pad;
            for (int rr = 0; rr < tms; rr++) {
                int64_t at0 = -1, ld = 0;                           // (the rows vbs_a8quant_kernel reads, see k_h16_a8.hip)
                if (rr < u.rows_lo) { at0 = u.off_lo + rr; ld = u.h_lo; }
                else if (rr >= 32 && rr - 32 < u.rows_hi) { at0 = u.off_hi + (rr - 32); ld = u.h_hi; }
                if (at0 < 0) continue;
                const int hf = rr >> 5;
                for (int k = 0; k < kp; k++) {
                    const int64_t i = at0 + (int64_t)k * ld;
                    if (i < 0 || i >= A->nztot) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": the slice map points outside the stored elements");
                    if (codes) codes[i] = img[(size_t)(s * slice + ((int64_t)(k / 8) * tms + rr) * 8 + (k & 7))];
                    if (exps) exps[i] = (int32_t)((word >> (16 * hf)) & 0xffffu) - 127;
                    if (group) group[i] = (int32_t)(s * (tms / 32) + hf);
                }
            }
        }
        return SPARTA_OK;
    });
    SPARTA_GUARD_END("sparta_vbs_a8_get")
}

namespace {

// the device state of an installed live set on the host (synchronises `st`)
struct LiveDownload { std::vector<uint8_t> keep; std::vector<int32_t> groups, gcount, tids, tcount; };
int live_download(sparta_vbs_t* A, const char* entry, void* stream, LiveDownload& D) {
    return open_call(DeviceCall{entry, A, (hipStream_t)stream, true}, [&](hipStream_t st) -> int {
        if (g_capturing) return capture_refusal("read the live set back (synchronises)", entry);
        HIP_TRY(hipStreamSynchronize(st));
        auto get = [](auto& vec, const void* src, int64_t n) {
            vec.resize((size_t)n);
            return n > 0 ? hipMemcpy(vec.data(), src, (size_t)n * sizeof(vec[0]), hipMemcpyDeviceToHost) : hipSuccess;
        };
        HIP_TRY(get(D.keep, A->d_live_keep, A->nblocks));
        HIP_TRY(get(D.groups, A->d_live_groups, A->live_n_groups));
        HIP_TRY(get(D.gcount, A->d_live_gcount, A->n_brows));
        HIP_TRY(get(D.tids, A->d_live_tids, A->live_n_tlist));
        HIP_TRY(get(D.tcount, A->d_live_tcount, (A->create_flags & SPARTA_CREATE_TRANSPOSE) ? A->live_block_cols : 0));
        return SPARTA_OK;
    });
}

}  // namespace

extern "C" int sparta_vbs_live_info(sparta_vbs_t* A, int64_t* info_out, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_live_info";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!info_out) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": NULL argument");
    std::memset(info_out, 0, 8 * sizeof(int64_t));
    info_out[1] = A->nblocks;
    info_out[7] = A->live_steps ? 1 : 0;
    if (!A->live_on) return SPARTA_OK;
    LiveDownload D;
    if (int rc = live_download(A, entry, stream, D)) return rc;
    info_out[0] = 1;
    for (uint8_t k : D.keep) info_out[2] += k != 0;
    info_out[3] = A->live_n_groups;
    for (int32_t n : D.gcount) info_out[4] += n;
    info_out[5] = A->live_n_tlist;
    for (int32_t n : D.tcount) info_out[6] += n;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_live_info")
}

extern "C" int sparta_vbs_live_lists_get(sparta_vbs_t* A, int32_t* sd_groups, int32_t* sd_count, int32_t* t_blocks, int32_t* t_count, void* stream) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_live_lists_get";
    if (int rc = prune_handle_check(A, entry)) return rc;
    if (!A->live_on) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": no live set is installed");
    LiveDownload D;
    if (int rc = live_download(A, entry, stream, D)) return rc;
    if (sd_groups && !D.groups.empty()) std::memcpy(sd_groups, D.groups.data(), D.groups.size() * sizeof(int32_t));
    if (sd_count) {                              // per block-row of the handle; the device keeps the block-rows of height > 0 only
        size_t at = 0;
        for (int64_t ib = 0; ib < A->block_rows; ib++) sd_count[ib] = A->h_row_part[(size_t)ib + 1] > A->h_row_part[(size_t)ib] ? D.gcount[at++] : 0;
    }
    if (t_blocks && !D.tids.empty()) std::memcpy(t_blocks, D.tids.data(), D.tids.size() * sizeof(int32_t));
    if (t_count && !D.tcount.empty()) std::memcpy(t_count, D.tcount.data(), D.tcount.size() * sizeof(int32_t));
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_live_lists_get")
}

// ---- sparta_vbs_spmm_t (k_spmm_t.hip) ---------------------------------------------------------------------------------------------------
namespace {

int spmm_t_impl(sparta_vbs_t* A, const void* X, int64_t ldx, int32_t n_cols, float* Ct, int64_t ldo, int32_t accumulate, int32_t ptr_space, void* stream,
                float* dt_ms) {
    using sparta::fail;
    if (!A || !X || !Ct) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: NULL argument");
    if (n_cols <= 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: n_cols must be > 0");
    if (ptr_space != SPARTA_PTR_HOST && ptr_space != SPARTA_PTR_DEVICE) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: bad ptr_space");
    if (!(A->create_flags & SPARTA_CREATE_TRANSPOSE))
        return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm_t: the handle was not made with SPARTA_CREATE_TRANSPOSE (sparta_vbs_create_range_ex; handles of "
                                            "sparta_vbs_create_from_csr and sparta_vbs_create_transposed cannot take the flag)");
    if (ldx < A->rows || ldo < A->cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: ldx < rows or ldo < cols");
    if (ldx > (INT64_C(1) << 61) / n_cols || ldo > (INT64_C(1) << 61) / n_cols) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_vbs_spmm_t: ldx * n_cols or ldo * n_cols beyond 2^61");
    const bool h16 = A->dtype != SPARTA_F32;
    if (h16 && ptr_space == SPARTA_PTR_DEVICE && (ldx & 1)) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: 16-bit handles need an even ldx");
    if (h16 && ptr_space == SPARTA_PTR_DEVICE && ((uintptr_t)X % 4) != 0) return fail(SPARTA_ERR_INVALID, "sparta_vbs_spmm_t: 16-bit X must start on a 4-byte boundary");

    const DeviceCall call{"sparta_vbs_spmm_t", A, (hipStream_t)stream, ptr_space == SPARTA_PTR_DEVICE, dt_ms, "the product", A->ev0, A->ev1};
    return open_call(call, [&](hipStream_t st) -> int {
        const void* dX = X;
        float* dC = Ct;
        int64_t kx = ldx;
        const size_t x_elems = (size_t)ldx * (size_t)(n_cols - 1) + (size_t)A->rows, c_elems = (size_t)ldo * (size_t)(n_cols - 1) + (size_t)A->cols;
        if (ptr_space == SPARTA_PTR_HOST) {
            // host in, host out: X and Ct staged in one device buffer (Ct whole, so that its padding rows come back as they went); 16-bit handles round X on the device
            if (int rc = A->d_t_ws.ensure((x_elems + c_elems) * sizeof(float), A->retired)) return rc;
            float* ws = (float*)A->d_t_ws;
            HIP_TRY(hipMemcpyAsync(ws, X, x_elems * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ws + x_elems, Ct, c_elems * sizeof(float), hipMemcpyHostToDevice, st));
            dX = ws; dC = ws + x_elems;
            if (h16) {
                kx = (A->rows + 7) / 8 * 8;
                if (int rc = A->d_t_h16.ensure((size_t)kx * (size_t)n_cols * sizeof(uint16_t), A->retired)) return rc;
                launch_convert_h16(A->dtype == SPARTA_BF16, st, ws, ldx, A->rows, n_cols, (uint16_t*)A->d_t_h16, kx);
                HIP_TRY(hipGetLastError());
                dX = A->d_t_h16;
            }
        }
        SpmmTParams p;
        p.items = A->d_t_items; p.blocks = A->d_t_blocks;
        if (A->live_on) { p.items = A->d_live_t_items; p.blocks = A->d_live_t_blocks; }      // the same kernels on the compacted lists (an empty list writes the zeros)
        p.A = h16 ? (const void*)A->d_t_A : (const void*)A->d_A;
        p.X = dX; p.Ct = dC;
        p.ldx = kx; p.ldo = ldo; p.cols = A->cols;
        p.n_cols = n_cols; p.w = (int32_t)A->w; p.accumulate = accumulate != 0; p.pad = 0;
        if (int rc = timed_launches(call, [&](hipStream_t) { launch_spmm_t(A->dtype, (unsigned)A->n_t_items, st, p); })) return rc;
        if (ptr_space == SPARTA_PTR_HOST) {
            HIP_TRY(hipMemcpyAsync(Ct, dC, c_elems * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return SPARTA_OK;
    });
}

}  // namespace

extern "C" int sparta_vbs_spmm_t(sparta_vbs_t* A, const void* X, int64_t ldx, int32_t n_cols, float* Ct, int64_t ldo, int32_t accumulate, int32_t ptr_space,
                                 void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    return spmm_t_impl(A, X, ldx, n_cols, Ct, ldo, accumulate, ptr_space, stream, dt_ms);
    SPARTA_GUARD_END("sparta_vbs_spmm_t")
}
