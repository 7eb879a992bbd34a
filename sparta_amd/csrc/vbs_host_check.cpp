// vbs_host_check.cpp -- the entries that make no HIP call: what the CPU suite checks the host builders and the host forms of the device rules with.
// sparta_colres_host_check, sparta_sparse_rows_host_check, sparta_union_host_check and sparta_spmm_t_host_check build an image the way creation builds it and
// walk it on the host the way its kernel walks it; sparta_vbs_block_table_host, sparta_vbs_repattern_host, sparta_vbs_live_lists_host,
// sparta_live_forward_compact, sparta_a8_quantize_group, sparta_f32_pack_blocks and sparta_frag_positions are the pattern and number rules alone.
// Kernels: none (the rules it shares with them are in vbs_kernel_common.hpp, vbs_plan.cpp and vbs_union.cpp).
// From vbs_host.hpp: SPARTA_GUARD_BEGIN / _END, order_sparse_rows and build_colres (vbs_capi.cpp).
#include "vbs_host.hpp"

using namespace sparta_dev;

extern "C" {

// the packing rule of the packed plan (f32_pack_blocks, vbs_kernel_common.hpp) for the CPU suite: no GPU involved
int sparta_f32_pack_blocks(int32_t n_blocks, const uint8_t* group_masks, int32_t* step_of_block, int32_t* slot0_of_block, int32_t* n_steps) {
    if (n_blocks < 0 || !n_steps || (n_blocks > 0 && (!group_masks || !step_of_block || !slot0_of_block)))
        return sparta::fail(SPARTA_ERR_INVALID, "sparta_f32_pack_blocks: bad argument");
    *n_steps = f32_pack_blocks(n_blocks, group_masks, step_of_block, slot0_of_block);
    return SPARTA_OK;
}

// the k-compaction rule of the fp32 fragment image (frag_position / frag_pairs, vbs_kernel_common.hpp) for the CPU suite: no GPU involved
int sparta_frag_positions(const uint8_t* nonempty, uint8_t* pos, int32_t* pairs) {
    if (!nonempty || !pos || !pairs) return sparta::fail(SPARTA_ERR_INVALID, "sparta_frag_positions: NULL argument");
    uint32_t mask = 0;
    for (int k = 0; k < 32; k++) mask |= (uint32_t)(nonempty[k] != 0) << k;
    for (int k = 0; k < 32; k++) pos[k] = (uint8_t)frag_position(mask, k);
    *pairs = frag_pairs(mask);
    return SPARTA_OK;
}

// the resident-column image of a CSR matrix, built and walked on the HOST exactly as k_colres.hip walks it (slots in slice order, the sums of a slot in entry order,
// extra cells added to their row in chunk order) for ONE column x of B: what the CPU suite checks the builder with (no GPU involved; not a product path)
int sparta_colres_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* crow, const float* x, float* y,
                             int64_t* info) {
    using sparta::fail;
    SPARTA_GUARD_BEGIN
    if (rows <= 0 || cols <= 0 || !rowptr || !colidx || !vals || !x || !y || !info) return fail(SPARTA_ERR_INVALID, "sparta_colres_host_check: bad argument");
    // crow[i] = the row of C of CSR row i (NULL: i); + 2^31: the row ADDS to y (a mixed block-row's sparse part); -1: CSR row i is not a sparse row (its row of C belongs to tiles: y untouched)
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci, cr;
    std::vector<float> va;
    for (int64_t i = 0; i < rows; i++) {
        if (crow && crow[i] == -1) continue;
        ci.insert(ci.end(), colidx + rowptr[i], colidx + rowptr[i + 1]);
        va.insert(va.end(), vals + rowptr[i], vals + rowptr[i + 1]);
        rp.push_back((int64_t)ci.size());
        cr.push_back(crow ? (int32_t)(uint32_t)(crow[i] & 0xffffffffll) : (int32_t)i);
    }
    ColresHost H;
    for (int k = 0; k < 12; k++) info[k] = 0;
    const int force_parts = [] { const char* e = std::getenv("SPARTA_COLRES_FORCE_PARTS"); return e ? atoi(e) : 0; }();      // (4: the image a handle keeps for products of few column sets)
    if (!build_colres(rows, cols, rp, ci, va, cr, H, force_parts)) return SPARTA_OK;    // info[0] = 0: this matrix gets no image
    const int n_ranges = (int)H.krange.size() - 1;
    for (const ColresPartDev& pd : H.parts) {
        const int32_t* wslice = H.meta.data() + pd.meta;
        const int32_t* woff = wslice + 17;
        const int32_t* bnd = woff + (size_t)n_ranges * 17;
        std::vector<float> acc((size_t)pd.n_slices * 64, 0.0f), cell((size_t)pd.plane, 0.0f);
        for (int r = 0; r < n_ranges; r++) {                                          // the sums of a slot carry over from range to range, as the kernel's registers do
            const int64_t k0 = H.krange[(size_t)r], klen = H.krange[(size_t)r + 1] - k0;
            for (int w = 0; w < kColresWaves; w++) {
                for (int32_t i = wslice[w]; i < wslice[w + 1]; i++) {
                    const int32_t t0 = i == wslice[w] ? 0 : bnd[(size_t)r * pd.n_slices + i - 1], t1 = bnd[(size_t)r * pd.n_slices + i];      // batches of 4 steps
                    if (t1 <= t0) return fail(SPARTA_ERR_INVALID, "sparta_colres_host_check: an empty slice in the image");
                    for (int l = 0; l < 64; l++) {
                        float a = acc[(size_t)i * 64 + (size_t)l];
                        for (int32_t t = t0; t < t1; t++) {
                            for (int u = 0; u < 4; u++) {
                                const size_t at = ((size_t)(woff[(size_t)r * 17 + w] + t) * 64 + (size_t)l) * 4 + (size_t)u;
                                const int64_t c = H.col[at];
                                if (c > klen) return fail(SPARTA_ERR_INVALID, "sparta_colres_host_check: column out of range in the image");
                                const float b = c == klen ? 0.0f : x[k0 + c];           // the zero cell behind the range's last row of B
                                a = H.val.empty() ? a + b : std::fma(H.val[at], b, a);
                            }
                        }
                        acc[(size_t)i * 64 + (size_t)l] = a;
                    }
                }
                if (wslice[w + 1] > wslice[w] && (int64_t)bnd[(size_t)r * pd.n_slices + wslice[w + 1] - 1] != (int64_t)woff[(size_t)r * 17 + w + 1] - woff[(size_t)r * 17 + w])
                    return fail(SPARTA_ERR_INVALID, "sparta_colres_host_check: a wave's stream and its slice boundaries disagree");
            }
        }
        for (int32_t q = 0; q < pd.n_slices * 64; q++) {
            const int32_t d = H.dest[(size_t)pd.dest + (size_t)q];
            if (d >= pd.plane) return fail(SPARTA_ERR_INVALID, "sparta_colres_host_check: cell out of range in the image");
            if (d >= 0) cell[(size_t)d] = acc[(size_t)q];
        }
        for (int32_t q = 0; q < pd.n_long; q++) {
            const ColresLong& lr = H.longs[(size_t)pd.longs + (size_t)q];
            float sum = cell[(size_t)lr.row];
            for (int32_t i = 0; i < lr.n; i++) sum += cell[(size_t)lr.first + (size_t)i];
            cell[(size_t)lr.row] = sum;
        }
        for (int32_t i = 0; i < pd.rows; i++) {
            const uint8_t m = H.mode[(size_t)(pd.r0 + i)];
            if (m == 1) y[pd.r0 + i] = cell[(size_t)i]; else if (m == 2) y[pd.r0 + i] += cell[(size_t)i];
        }
    }
    info[0] = H.max_slices; info[1] = H.entries; info[2] = (int64_t)H.longs.size(); info[3] = H.max_cells; info[4] = H.lmax; info[6] = rp.back(); info[7] = H.val.empty() ? 1 : 0;
    info[8] = (int64_t)H.parts.size(); info[9] = n_ranges;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_colres_host_check")
}

// the sparse-row device form of a CSR matrix (order_sparse_rows), built and walked on the HOST as the kernels of k_sparse.hip walk it for ONE column x of B: the short
// rows from the list, a long row through its record -- its segments in row order, one partial per segment at the segment's `pad`, the partials added in that order.
// What the CPU suite checks the builder with (no GPU involved; not a product path).  crow: as for sparta_colres_host_check.
// info: [0] sparse rows, [1] short rows, [2] long rows, [3] segments, [4] window width (0: off), [5] streams with segments (0: one list), [6] base segment length,
// [7] longest short row, [8] SPARTA_SP_MINSEG as resolved
int sparta_sparse_rows_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* crow, const float* x, float* y,
                                  int64_t* info) {
    using sparta::fail;
    SPARTA_GUARD_BEGIN
    if (rows <= 0 || cols <= 0 || !rowptr || !colidx || !vals || !x || !y || !info) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: bad argument");
    // the walk below indexes x by column and y by crow: a CSR that is not one comes back as an error, not as a read out of bounds
    if (rowptr[0] != 0) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: rowptr must start at 0");
    for (int64_t i = 0; i < rows; i++) {
        if (rowptr[i + 1] < rowptr[i]) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: rowptr is not monotone");
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++)
            if (colidx[k] < 0 || colidx[k] >= cols) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: column index out of range");
        if (crow && crow[i] != -1 && (crow[i] < 0 || (crow[i] & 0x7fffffffll) >= rows || (crow[i] >> 32) != 0))
            return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: crow entry out of range");
    }
    SparseRowsHost S;
    S.rowptr.push_back(0);
    for (int64_t i = 0; i < rows; i++) {
        if (crow && crow[i] == -1) continue;
        S.col.insert(S.col.end(), colidx + rowptr[i], colidx + rowptr[i + 1]);
        S.val.insert(S.val.end(), vals + rowptr[i], vals + rowptr[i + 1]);
        S.rowptr.push_back((int64_t)S.col.size());
        S.crow.push_back(crow ? (int32_t)(uint32_t)(crow[i] & 0xffffffffll) : (int32_t)i);
    }
    for (int k = 0; k < 12; k++) info[k] = 0;
    if (int rc = order_sparse_rows(S, cols)) return rc;
    const int64_t n = (int64_t)S.crow.size(), n_segs = (int64_t)S.segs.size();
    std::vector<uint8_t> covered((size_t)S.rowptr.back(), 0), seen((size_t)n, 0);
    // entries [p0, p0 + cnt) of the CSR times x, each entry taken once
    auto dot = [&](int64_t p0, int64_t cnt, float& sum) -> bool {
        if (p0 < 0 || cnt < 0 || p0 + cnt > S.rowptr.back()) return false;
        for (int64_t k = p0; k < p0 + cnt; k++) {
            if (covered[(size_t)k]++) return false;
            sum = std::fma(S.val[(size_t)k], x[S.col[(size_t)k]], sum);
        }
        return true;
    };
    auto finish = [&](int64_t t, float sum) { const int32_t c = S.crow[(size_t)t]; if (c < 0) y[c & 0x7fffffff] += sum; else y[c] = sum; };
    for (const int32_t t : S.list) {
        if (t < 0 || t >= n || seen[(size_t)t]++) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a list entry is no row, or a row is taken twice");
        if (S.rowptr[(size_t)t + 1] - S.rowptr[(size_t)t] > S.long_cut) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a long row in the list of short rows");
        float sum = 0.0f;
        if (!dot(S.rowptr[(size_t)t], S.rowptr[(size_t)t + 1] - S.rowptr[(size_t)t], sum)) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a nonzero is covered twice");
        finish(t, sum);
    }
    std::vector<int64_t> at_pad((size_t)n_segs, -1);                                  // segment in row order -> its place in the list
    for (int64_t i = 0; i < n_segs; i++) {
        const int32_t p = S.segs[(size_t)i].pad;
        if (p < 0 || p >= n_segs || at_pad[(size_t)p] >= 0) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: pad is not a permutation of the segments");
        at_pad[(size_t)p] = i;
    }
    std::vector<float> partial((size_t)n_segs, 0.0f);
    int64_t segs_of_rows = 0;
    for (const SpLongRec& lr : S.longs) {
        if (lr.ord < 0 || lr.ord >= n || seen[(size_t)lr.ord]++) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a long record is no row, or a row is taken twice");
        if (lr.n_seg <= 0 || lr.seg_begin != segs_of_rows || (int64_t)lr.seg_begin + lr.n_seg > n_segs)
            return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: the segments of the long rows are not back to back in row order");
        int64_t next = S.rowptr[(size_t)lr.ord];
        float sum = 0.0f;
        for (int32_t q = lr.seg_begin; q < lr.seg_begin + lr.n_seg; q++) {
            const SpSegRec& g = S.segs[(size_t)at_pad[(size_t)q]];
            if (g.p0 != next || g.cnt <= 0) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a row's segments are not contiguous and in order");
            if (!dot(g.p0, g.cnt, partial[(size_t)q])) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a nonzero is covered twice");
            next = g.p0 + g.cnt;
            sum += partial[(size_t)q];
        }
        if (next != S.rowptr[(size_t)lr.ord + 1]) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a row's segments do not end at the row's end");
        segs_of_rows += lr.n_seg;
        finish(lr.ord, sum);
    }
    if (segs_of_rows != n_segs) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a segment belongs to no long row");
    for (int64_t t = 0; t < n; t++) if (!seen[(size_t)t]) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a row is neither short nor long");
    for (const uint8_t c : covered) if (c != 1) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a nonzero is not covered");
    // the order the waves take the segments in: window by window (one list), or per stream (XCD order)
    auto window_of = [&](int64_t i) { return (int64_t)S.col[(size_t)S.segs[(size_t)i].p0] / S.win_w; };
    int64_t streams_used = 0;
    if (!S.stream_begin.empty()) {
        const std::vector<int32_t>& sb = S.stream_begin;
        if (S.win_w <= 0 || sb.size() != 9 || sb[0] != 0 || sb[8] != n_segs) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: stream_begin does not span the segments");
        std::vector<int8_t> stream_of((size_t)((cols + S.win_w - 1) / S.win_w), -1);
        for (int s = 0; s < 8; s++) {
            if (sb[(size_t)s + 1] < sb[(size_t)s]) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: stream_begin is not monotone");
            streams_used += sb[(size_t)s + 1] > sb[(size_t)s];
            for (int64_t i = sb[(size_t)s]; i < sb[(size_t)s + 1]; i++) {
                const int64_t k = window_of(i);
                if (stream_of[(size_t)k] >= 0 && stream_of[(size_t)k] != s) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a window's segments are split across streams");
                stream_of[(size_t)k] = (int8_t)s;
                if (i > sb[(size_t)s] && window_of(i - 1) > k) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: a stream's windows are not in column order");
            }
        }
    } else if (S.win_w > 0) {
        for (int64_t i = 1; i < n_segs; i++)
            if (window_of(i - 1) > window_of(i)) return fail(SPARTA_ERR_INVALID, "sparta_sparse_rows_host_check: the segments are not in window order");
    }
    info[0] = n; info[1] = (int64_t)S.list.size(); info[2] = (int64_t)S.longs.size(); info[3] = n_segs; info[4] = S.win_w; info[5] = streams_used;
    info[6] = S.seg; info[7] = S.long_cut; info[8] = S.minseg;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_sparse_rows_host_check")
}

// the hybrid image of a CSR matrix under `grouping`, built exactly as sparta_vbs_create_from_csr builds it for an fp32 handle -- w-wide tiles, column-compacted tiles,
// sparse rows -- and multiplied with ONE column x on the HOST: the w-wide tiles from the reference-layout image, the column-compacted tiles by walking their DEVICE
// form (per-worker step records, list entries, fragment-order slices: vbs_union.cpp), the sparse rows entry by entry.  What the CPU suite checks the mode-3 builder
// and the plan with (no GPU involved; not a product path).  y: [padded rows], reordered order, double.
int sparta_union_host_check(int64_t rows, int64_t cols, const int64_t* rowptr, const int32_t* colidx, const float* vals, const int64_t* grouping, int64_t col_block_size,
                            int64_t row_block_size, int32_t force_fixed_size, int32_t max_workers, const float* x, double* y, int64_t* info) {
    using sparta::fail;
    SPARTA_GUARD_BEGIN
    if (!rowptr || !colidx || !grouping || !x || !y || !info || max_workers <= 0) return fail(SPARTA_ERR_INVALID, "sparta_union_host_check: bad argument");
    sparta::CsrView a;
    a.rows = rows; a.cols = cols; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
    double K = 24.0;
    if (const char* e = std::getenv("SPARTA_SPARSE_K")) K = atof(e);
    if (!(K > 0.0)) return fail(SPARTA_ERR_INVALID, "sparta_union_host_check: the hybrid builder is switched off (SPARTA_SPARSE_K=0)");
    sparta::HybridSparse sp;
    sp.esz = 4.0; sp.want_union = true; sp.union_gran = 16;
    sparta_vbs_host h;
    std::memset(&h, 0, sizeof(h));
    struct Free { sparta_vbs_host* p; ~Free() { sparta_vbs_host_free(p); } } guard{&h};
    if (int rc = sparta::vbs_build_hybrid(a, grouping, col_block_size, row_block_size, force_fixed_size != 0, K, 32, &h, &sp)) return rc;
    for (int64_t r = 0; r < h.rows; r++) y[r] = 0.0;
    int64_t jo = 0, mo = 0;
    for (int64_t ib = 0; ib < h.block_rows; ib++) {                       // the w-wide tiles
        const int64_t r0 = h.row_part[ib], hh = h.row_part[ib + 1] - r0;
        for (int64_t b = 0; b < h.nzcount[ib]; b++, jo++, mo += hh * col_block_size)
            for (int64_t k = 0; k < col_block_size && h.jab[jo] * col_block_size + k < cols; k++)
                for (int64_t i = 0; i < hh; i++) y[r0 + i] += (double)h.mab[mo + k * hh + i] * (double)x[h.jab[jo] * col_block_size + k];
    }
    UnionDevPlan P;
    if (!sp.uni.empty()) {
        if (int rc = build_union_plan(sp.uni, max_workers, P)) return rc;
        union_plan_host_apply(P, x, y);
    }
    for (size_t t = 0; t < sp.crow.size(); t++)                           // the sparse rows (they own their row or add to it: y started at zero either way)
        for (int64_t k = sp.rowptr[t]; k < sp.rowptr[t + 1]; k++) y[sp.crow[t]] += (double)sp.val[(size_t)k] * (double)x[sp.col[(size_t)k]];
    info[0] = (int64_t)sp.uni.tiles[0].size(); info[1] = (int64_t)sp.uni.tiles[1].size(); info[2] = P.steps_by_height[0]; info[3] = P.steps_by_height[1];
    info[4] = P.area; info[5] = P.cols; info[6] = sp.uni.nnz; info[7] = sp.rowptr.empty() ? 0 : sp.rowptr.back();
    info[8] = h.nztot; info[9] = h.rows; info[10] = std::max(P.n_workers[0], P.n_workers[1]); info[11] = std::max(P.n_workers[2], P.n_workers[3]); info[12] = sp.uni.tail_nnz; info[13] = P.rows;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_union_host_check")
}

int sparta_vbs_block_table_host(int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t br0,
                                           int64_t br1, int64_t* table_out, int64_t* n_blocks_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount || !n_blocks_out)
        return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_table_host: bad dimensions or NULL argument");
    if (br0 < 0 || br1 > block_rows || br0 > br1) return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_table_host: bad block-row range");
    const int64_t block_cols = (cols - 1) / w + 1;
    int64_t jab_lo = 0, nblocks = 0;
    for (int64_t ib = 0; ib < br1; ib++) {
        if (row_part[ib + 1] < row_part[ib] || nzcount[ib] < 0 || nzcount[ib] > block_cols) return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_table_host: invalid row_part / nzcount");
        if (ib < br0) jab_lo += nzcount[ib];
        else nblocks += nzcount[ib];
    }
    if (nblocks > 0 && table_out && !jab) return fail(SPARTA_ERR_INVALID, "sparta_vbs_block_table_host: jab is NULL");
    return build_block_table(cols, w, br0, br1, row_part, nzcount, jab, jab_lo, table_out, n_blocks_out);
    SPARTA_GUARD_END("sparta_vbs_block_table_host")
}

// Everything is validated before the first output is written: an INVALID call leaves the caller's arrays as they were.
int sparta_vbs_repattern_host(int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t br0,
                                         int64_t br1, const uint8_t* keep, const int64_t* add, int64_t n_add, int64_t* nzcount_out, int64_t* jab_out,
                                         int32_t* map_out, int64_t* counts_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* me = "sparta_vbs_repattern_host";
    if (cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount || !counts_out || n_add < 0)
        return fail(SPARTA_ERR_INVALID, std::string(me) + ": bad dimensions or NULL argument");
    if (br0 < 0 || br1 > block_rows || br0 > br1) return fail(SPARTA_ERR_INVALID, std::string(me) + ": bad block-row range");
    if (n_add > 0 && !add) return fail(SPARTA_ERR_INVALID, std::string(me) + ": add is NULL with n_add > 0");
    const int64_t block_cols = (cols - 1) / w + 1;
    int64_t jab_lo = 0, n_range = 0, n_after = 0, nz_outside = 0;
    for (int64_t ib = 0; ib < block_rows; ib++) {
        if (row_part[ib + 1] < row_part[ib] || nzcount[ib] < 0 || nzcount[ib] > block_cols) return fail(SPARTA_ERR_INVALID, std::string(me) + ": invalid row_part / nzcount");
        if (ib < br0) jab_lo += nzcount[ib];
        else if (ib < br1) n_range += nzcount[ib];
        else n_after += nzcount[ib];
        if (ib < br0 || ib >= br1) nz_outside += nzcount[ib] * (row_part[ib + 1] - row_part[ib]) * w;
    }
    if (jab_lo + n_range + n_after > 0 && !jab) return fail(SPARTA_ERR_INVALID, std::string(me) + ": jab is NULL");
    // the old pattern of the range: strictly ascending block columns inside [0, block_cols)
    for (int64_t ib = br0, q = jab_lo; ib < br1; ib++)
        for (int64_t b = 0; b < nzcount[ib]; b++, q++) {
            if (jab[q] < 0 || jab[q] >= block_cols) return fail(SPARTA_ERR_INVALID, std::string(me) + ": jab entry out of range");
            if (b > 0 && jab[q] <= jab[q - 1]) return fail(SPARTA_ERR_INVALID, std::string(me) + ": jab is not strictly ascending inside a block-row of the range");
        }
    // the added blocks, sorted by (block-row, block column): inside the range, inside the matrix, each once, none stored already
    std::vector<std::pair<int64_t, int64_t>> adds((size_t)n_add);
    for (int64_t a = 0; a < n_add; a++) {
        adds[(size_t)a] = {add[2 * a], add[2 * a + 1]};
        if (add[2 * a] < br0 || add[2 * a] >= br1) return fail(SPARTA_ERR_INVALID, std::string(me) + ": an added block lies outside the block-row range");
        if (add[2 * a + 1] < 0 || add[2 * a + 1] >= block_cols) return fail(SPARTA_ERR_INVALID, std::string(me) + ": an added block has a block column outside the matrix");
    }
    std::sort(adds.begin(), adds.end());
    for (size_t a = 1; a < adds.size(); a++)
        if (adds[a] == adds[a - 1]) return fail(SPARTA_ERR_INVALID, std::string(me) + ": an added block is given twice");
    std::vector<int64_t> row_first((size_t)(br1 - br0) + 1, 0);          // first old block (numbered in the range) of every block-row of the range
    for (int64_t ib = br0; ib < br1; ib++) row_first[(size_t)(ib - br0) + 1] = row_first[(size_t)(ib - br0)] + nzcount[ib];
    for (const auto& ad : adds) {
        const int64_t* lo = jab + jab_lo + row_first[(size_t)(ad.first - br0)];
        const int64_t* hi = jab + jab_lo + row_first[(size_t)(ad.first - br0) + 1];
        if (std::binary_search(lo, hi, ad.second))
            return fail(SPARTA_ERR_INVALID, std::string(me) + ": an added block is stored by the old pattern (a stored dead block comes back through keep)");
    }
    // counts
    int64_t new_range = n_add, nz_range = 0;
    {
        size_t a = 0;
        for (int64_t ib = br0; ib < br1; ib++) {
            int64_t n = 0;
            for (int64_t q = row_first[(size_t)(ib - br0)]; q < row_first[(size_t)(ib - br0) + 1]; q++) n += !keep || keep[q] != 0;
            new_range += n;
            while (a < adds.size() && adds[a].first == ib) { n++; a++; }
            nz_range += n * (row_part[ib + 1] - row_part[ib]) * w;
        }
    }
    if (new_range > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(me) + ": more than 2^31 - 1 blocks in the new range");
    const int64_t new_total = jab_lo + new_range + n_after;
    const bool count_only = !jab_out && !map_out;
    if (!count_only) {
        if (!nzcount_out) return fail(SPARTA_ERR_INVALID, std::string(me) + ": nzcount_out is NULL");
        if ((!jab_out && new_total > 0) || (!map_out && new_range > 0)) return fail(SPARTA_ERR_INVALID, std::string(me) + ": jab_out or map_out is NULL");
    }
    // ---- nothing was written up to here ----
    counts_out[0] = new_total; counts_out[1] = nz_outside + nz_range; counts_out[2] = new_range; counts_out[3] = nz_range;
    if (nzcount_out) {
        size_t a = 0;
        for (int64_t ib = 0; ib < block_rows; ib++) {
            int64_t n = nzcount[ib];
            if (ib >= br0 && ib < br1) {
                n = 0;
                for (int64_t q = row_first[(size_t)(ib - br0)]; q < row_first[(size_t)(ib - br0) + 1]; q++) n += !keep || keep[q] != 0;
                while (a < adds.size() && adds[a].first == ib) { n++; a++; }
            }
            nzcount_out[ib] = n;
        }
    }
    if (count_only) return SPARTA_OK;
    int64_t o = 0;
    for (int64_t q = 0; q < jab_lo; q++) jab_out[o++] = jab[q];
    {
        size_t a = 0;
        int64_t m = 0;
        for (int64_t ib = br0; ib < br1; ib++) {
            int64_t q = row_first[(size_t)(ib - br0)];
            const int64_t q1 = row_first[(size_t)(ib - br0) + 1];
            for (;;) {                                                    // merge of two ascending lists that share no column
                while (q < q1 && keep && keep[q] == 0) q++;
                const bool has_add = a < adds.size() && adds[a].first == ib;
                if (q >= q1 && !has_add) break;
                if (has_add && (q >= q1 || adds[a].second < jab[jab_lo + q])) {
                    jab_out[o++] = adds[a].second; map_out[m++] = -1; a++;
                } else {
                    jab_out[o++] = jab[jab_lo + q]; map_out[m++] = (int32_t)q; q++;
                }
            }
        }
    }
    for (int64_t q = jab_lo + n_range; q < jab_lo + n_range + n_after; q++) jab_out[o++] = jab[q];
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_repattern_host")
}

int sparta_a8_quantize_group(const float* v, int64_t ld, int32_t rows, int32_t kcols, uint8_t* codes, int32_t* e_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_a8_quantize_group";
    if (rows < 0 || rows > 32 || (kcols != 32 && kcols != 64) || ld < rows || !e_out || (rows > 0 && (!v || !codes)))
        return fail(SPARTA_ERR_INVALID, std::string(entry) + ": rows must lie in 0..32, kcols be 32 or 64, ld >= rows, and no pointer be NULL");
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    uint32_t amax = 0;
    for (int32_t k = 0; k < kcols; k++)
        for (int32_t r = 0; r < rows; r++) amax = a8_amax_bits(amax, bits(v[(int64_t)k * ld + r]));
    const int32_t e = a8_exponent(amax);
    const uint32_t inv_bits = a8_inv_scale_bits(e);
    float inv;
    std::memcpy(&inv, &inv_bits, 4);
    for (int32_t k = 0; k < kcols; k++)
        for (int32_t r = 0; r < rows; r++) {
            volatile float x = v[(int64_t)k * ld + r] * inv;      // (one fp32 multiplication, as the kernel's)
            codes[(int64_t)k * rows + r] = (uint8_t)a8_code(bits(x));
        }
    *e_out = e;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_a8_quantize_group")
}

int sparta_live_forward_compact(const void* steps, int64_t n_steps, const int32_t* ranges, int64_t n_ranges, int32_t pair_image, const uint8_t* live,
                                           void* steps_out, int32_t* ranges_out, int64_t* info_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_live_forward_compact";
    if (n_steps < 0 || n_ranges < 0 || !info_out || (n_steps > 0 && (!steps || !live || !steps_out)) || (n_ranges > 0 && (!ranges || !ranges_out)))
        return fail(SPARTA_ERR_INVALID, std::string(entry) + ": bad sizes or NULL argument");
    if (n_steps > INT32_MAX) return fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": more than 2^31 - 1 steps");
    for (int64_t r = 0; r < n_ranges; r++)
        if (ranges[2 * r] < 0 || ranges[2 * r + 1] > n_steps)
            return fail(SPARTA_ERR_INVALID, std::string(entry) + ": a range lies outside the records");
    int64_t info[8];
    live_forward_compact_host((const StepRec*)steps, n_steps, ranges, n_ranges, pair_image != 0, live, (StepRec*)steps_out, ranges_out, info);
    std::memcpy(info_out, info, sizeof(info));
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_live_forward_compact")
}

int sparta_vbs_live_lists_host(int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t br0,
                                          int64_t br1, const uint8_t* keep, int32_t* sd_groups, int32_t* sd_count, int32_t* t_blocks, int32_t* t_count, int64_t* info_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const char* entry = "sparta_vbs_live_lists_host";
    if (cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount || !info_out) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": bad dimensions or NULL argument");
    if (br0 < 0 || br1 > block_rows || br0 > br1) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": bad block-row range");
    const int64_t block_cols = (cols - 1) / w + 1;
    int64_t jab_lo = 0, nblocks = 0;
    for (int64_t ib = 0; ib < br1; ib++) {
        if (row_part[ib + 1] < row_part[ib] || nzcount[ib] < 0 || nzcount[ib] > block_cols) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": invalid row_part / nzcount");
        if (ib < br0) jab_lo += nzcount[ib];
        else nblocks += nzcount[ib];
    }
    if (nblocks > 0 && (!jab || !keep)) return fail(SPARTA_ERR_INVALID, std::string(entry) + ": jab or keep is NULL");
    LiveMapsHost M;
    if (int rc = build_live_maps(cols, w, br0, br1, row_part, nzcount, jab, jab_lo, M)) return rc;
    std::vector<int32_t> g((size_t)M.goff.back()), gc((size_t)(br1 - br0)), t((size_t)M.tptr.back()), tc((size_t)block_cols);
    live_lists_host(M, keep, g.data(), gc.data(), t.data(), tc.data(), info_out);
    if (sd_groups && !g.empty()) std::memcpy(sd_groups, g.data(), g.size() * sizeof(int32_t));
    if (sd_count && !gc.empty()) std::memcpy(sd_count, gc.data(), gc.size() * sizeof(int32_t));
    if (t_blocks && !t.empty()) std::memcpy(t_blocks, t.data(), t.size() * sizeof(int32_t));
    if (t_count) std::memcpy(t_count, tc.data(), tc.size() * sizeof(int32_t));
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_vbs_live_lists_host")
}

// the block-column index of sparta_vbs_spmm_t, built by the function create calls and walked on the HOST the way k_spmm_t.hip walks it (an item's stored columns,
// each summed over the item's list in list order) for one vector: what the CPU suite checks the builder with (no GPU involved; not a product path)
int sparta_spmm_t_host_check(int64_t rows, int64_t cols, int64_t block_rows, int64_t w, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab,
                                        const float* mab, int64_t br0, int64_t br1, const float* x, double* y, int64_t* info_out) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    if (rows <= 0 || cols <= 0 || block_rows <= 0 || w <= 0 || !row_part || !nzcount || !x || !y || !info_out)
        return fail(SPARTA_ERR_INVALID, "sparta_spmm_t_host_check: bad dimensions or NULL argument");
    if (br0 < 0 || br1 > block_rows || br0 >= br1) return fail(SPARTA_ERR_INVALID, "sparta_spmm_t_host_check: bad block-row range");
    if (row_part[0] != 0 || row_part[block_rows] != rows) return fail(SPARTA_ERR_INVALID, "sparta_spmm_t_host_check: row_part must span [0, rows]");
    const int64_t block_cols = (cols - 1) / w + 1;
    int64_t jab_lo = 0, mab_lo = 0, nblocks = 0;
    for (int64_t ib = 0; ib < br1; ib++) {
        const int64_t h = row_part[ib + 1] - row_part[ib];
        if (h < 0 || nzcount[ib] < 0 || nzcount[ib] > block_cols) return fail(SPARTA_ERR_INVALID, "sparta_spmm_t_host_check: invalid row_part / nzcount");
        if (ib < br0) { jab_lo += nzcount[ib]; mab_lo += nzcount[ib] * h * w; }
        else nblocks += nzcount[ib];
    }
    if (nblocks > 0 && (!jab || !mab)) return fail(SPARTA_ERR_INVALID, "sparta_spmm_t_host_check: jab / mab is NULL");
    SpmmTIndexHost T;
    if (int rc = build_spmm_t_index(cols, w, br0, br1, row_part, nzcount, jab, jab_lo, false, T)) return rc;
    for (int64_t c = 0; c < cols; c++) y[c] = 0.0;
    for (const SpmmTItem& it : T.items)
        for (int64_t q = it.q0; q < std::min<int64_t>(it.q0 + 32, w); q++) {
            const int64_t col = (int64_t)it.jb * w + q;
            if (col >= cols) continue;
            double sum = 0.0;
            for (int32_t l = it.l0; l < it.l1; l++) {
                const SpmmTBlock& b = T.blocks[(size_t)l];
                const float* a = mab + mab_lo + b.off + q * b.h;
                for (int32_t i = 0; i < b.h; i++) sum += (double)a[i] * (double)x[b.r0 + i];
            }
            y[col] = sum;
        }
    std::memset(info_out, 0, 8 * sizeof(int64_t));
    info_out[0] = T.cols_with_blocks; info_out[1] = (int64_t)T.items.size(); info_out[2] = T.max_list; info_out[3] = 0;
    return SPARTA_OK;
    SPARTA_GUARD_END("sparta_spmm_t_host_check")
}

}  // extern "C"
