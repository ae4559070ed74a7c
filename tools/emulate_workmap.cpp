// emulate_workmap.cpp - the work maps of deeppowers_amd/csrc/workmap.h on the CPU (TEST INFRASTRUCTURE, like emulate.cpp and emulate_reduce.cpp).
// Per map: "decode ids [0, n_ids)" with the very functions the kernels call, and "the grid for these parameters" with the very functions the launchers
// call.  Rows of `out` are int64.  Built by tests/test_work_maps_cpu.py (g++), never shipped.
#include "../deeppowers_amd/csrc/devtables.h"
#include "../deeppowers_amd/csrc/workmap.h"

using namespace dpfhe;
typedef long long i64;

namespace {
struct Tables {   // what the limb helpers of devtables.h read of a DevTables
    int n_sub, n_limbs, n_active;
    unsigned long long active_map;
};
template <int LOGN> void src_pos_all(unsigned g, i64* out) {
    for (unsigned p = 0; p < (1u << LOGN); ++p) out[p] = galois_src_pos<LOGN>(g, p);
}
}  // namespace

extern "C" {

// key switching: plan -> grid (n_outer through the pointer); rows (item, limb, live) - limb through the launch's active_map when n_active != 0
u64 wm_relin_plan(size_t blocks, unsigned La, size_t key_stride, unsigned key_group, unsigned* n_outer) {
    const RelinPlan p = RelinMap::plan(blocks, La, key_stride, key_group);
    *n_outer = p.n_outer;
    return p.grid;
}
void wm_relin_decode(unsigned n_ids, unsigned n_outer, unsigned key_group, unsigned La, int n_limbs, int n_active, unsigned long long active_map, i64* out) {
    const Tables tb{1, n_limbs, n_active, active_map};
    for (unsigned id = 0; id < n_ids; ++id) {
        const RelinWork w = RelinMap::decode(id, n_outer, key_group, La);
        out[3 * id] = (i64)w.item; out[3 * id + 1] = launch_limb(tb, (unsigned)w.limb_index); out[3 * id + 2] = w.live;
    }
}

// hoisted rotations: rows (rotation, limb index, component, token, live)
void wm_hoisted_plan(size_t count, unsigned La, size_t n_items, int merged, unsigned* tiles, unsigned* blocks) {
    const HoistedPlan p = HoistedMap::plan(count, La, n_items, merged != 0);
    *tiles = p.tiles;
    *blocks = p.blocks;
}
void wm_hoisted_decode(unsigned n_ids, unsigned n_items, unsigned n_tiles, unsigned La, int merged, i64* out) {
    for (unsigned id = 0; id < n_ids; ++id) {
        const HoistedWork w = merged ? HoistedMap::decode<true>(id, n_items, n_tiles, La) : HoistedMap::decode<false>(id, n_items, n_tiles, La);
        i64* o = out + 5 * (size_t)id;
        o[0] = (i64)w.rot; o[1] = w.limb_index; o[2] = w.comp; o[3] = w.token; o[4] = w.live;
    }
}

// matrix-vector products: rows (limb, chunk, row tile, group, live)
u64 wm_matvec_grid(size_t n_limbs, size_t chunks, size_t row_tiles, size_t n_groups) { return MatvecMap::grid(n_limbs, chunks, row_tiles, n_groups); }
void wm_matvec_decode(unsigned n_ids, unsigned n_limbs, unsigned chunks, unsigned row_tiles, unsigned n_groups, i64* out) {
    for (unsigned id = 0; id < n_ids; ++id) {
        const MatvecWork w = MatvecMap::decode(id, n_limbs, chunks, row_tiles, n_groups);
        i64* o = out + 5 * (size_t)id;
        o[0] = w.limb; o[1] = w.chunk; o[2] = w.row_tile; o[3] = w.group; o[4] = w.live;
    }
}

// baby steps: rows (limb, source segment, rotation, token, live); pair map of one (g, source segment): rows (out, src, swap, ok) per lane
u64 wm_qp_grid(int log2n, size_t n_limbs, size_t n_rot, size_t n_items, unsigned pairs) { return QpMap::grid(log2n, n_limbs, n_rot, n_items, pairs); }
unsigned wm_qp_segments(int log2n, unsigned pairs) { return QpMap::geo(log2n, pairs).nseg; }
void wm_qp_decode(unsigned n_ids, int log2n, unsigned pairs, unsigned n_limbs, unsigned n_rot, unsigned n_items, i64* out) {
    const QpGeo geo = QpMap::geo(log2n, pairs);
    for (unsigned id = 0; id < n_ids; ++id) {
        const QpWork w = QpMap::decode(id, geo, n_limbs, n_rot, n_items);
        i64* o = out + 5 * (size_t)id;
        o[0] = w.limb; o[1] = w.sseg; o[2] = w.rot; o[3] = w.token; o[4] = w.live;
    }
}
void wm_qp_pair_map(int log2n, unsigned pairs, unsigned g, unsigned sseg, i64* out) {
    const QpGeo geo = QpMap::geo(log2n, pairs);
    for (unsigned lane = 0; lane < geo.seg_pairs; ++lane) {
        const QpPair p = QpMap::pair_map(g, sseg, lane, geo);
        i64* o = out + 4 * (size_t)lane;
        o[0] = p.out; o[1] = p.src; o[2] = p.swap; o[3] = p.ok;
    }
}

// streaming kernels: rows (chunk, limb, polynomial)
int wm_chunks_of(size_t n) { return chunks_of(n); }
void wm_chunk_decode(unsigned n_ids, int chunks, int n_limbs, i64* out) {
    for (unsigned id = 0; id < n_ids; ++id) {
        const ChunkWork w = chunk_work(id, chunks, n_limbs);
        out[3 * id] = w.chunk; out[3 * id + 1] = w.limb; out[3 * id + 2] = (i64)w.poly;
    }
}

// last pass of a relinearised product that also drops the last data prime (alone or with a linear combination): the grid; ids decode through wm_chunk_decode
// over the Ld - 1 kept limbs
u64 wm_relin_rescale_grid(size_t batch, size_t n_data_limbs, size_t n) { return relin_rescale_grid(batch, n_data_limbs, n); }
// a sum of tensor products: the grid; ids decode through wm_chunk_decode over all limbs, the group in the polynomial's place
u64 wm_mul_sum_grid(size_t groups, size_t n_limbs, size_t n) { return mul_sum_grid(groups, n_limbs, n); }
// products with a shared complement factor: the grid; ids decode through wm_chunk_decode over all limbs, the group in the polynomial's place
u64 wm_mul_complement_grid(size_t groups, size_t n_limbs, size_t n) { return mul_complement_grid(groups, n_limbs, n); }

// all pairs of resident and streamed operands: the grid of a launch over a_count resident ones, and per id the row (limb, chunk, tile, live, keys walked,
// rows of the tile); wm_mul_outer_pairs lists what ONE id writes, as the kernel's loops do: rows (output item, local row i, local key j), returns their number
int wm_mul_outer_tile() { return kMulOuterTile; }
u64 wm_mul_outer_grid(size_t a_count, size_t n_limbs, size_t n) { return MulOuterMap::grid(a_count, n_limbs, n); }
void wm_mul_outer_decode(unsigned n_ids, unsigned n_limbs, unsigned chunks, size_t a_count, size_t b_count, size_t a_off, size_t b_off, int causal, i64* out) {
    const unsigned tiles = (unsigned)MulOuterMap::tiles(a_count);
    for (unsigned id = 0; id < n_ids; ++id) {
        const MulOuterWork w = MulOuterMap::decode(id, tiles, n_limbs, chunks);
        i64* o = out + 6 * (size_t)id;
        const size_t r0 = w.tile * kMulOuterTile;
        o[0] = w.limb; o[1] = w.chunk; o[2] = (i64)w.tile; o[3] = w.live;
        o[4] = w.live ? (i64)MulOuterMap::keys(r0, a_count, b_count, a_off, b_off, causal != 0) : 0;
        o[5] = w.live ? (i64)(a_count - r0 < (size_t)kMulOuterTile ? a_count - r0 : (size_t)kMulOuterTile) : 0;
    }
}
size_t wm_mul_outer_pairs(size_t tile, size_t a_count, size_t b_count, size_t a_off, size_t b_off, size_t b_total, int causal, i64* out) {
    const size_t r0 = tile * kMulOuterTile, keys = MulOuterMap::keys(r0, a_count, b_count, a_off, b_off, causal != 0);
    const size_t rows = a_count - r0 < (size_t)kMulOuterTile ? a_count - r0 : (size_t)kMulOuterTile;
    size_t m = 0;
    for (size_t j = 0; j < keys; ++j)
        for (size_t t = 0; t < rows; ++t) {
            if (!MulOuterMap::writes(r0 + t, j, a_off, b_off, causal != 0)) continue;
            out[3 * m] = (i64)MulOuterMap::item(r0 + t, j, a_off, b_off, b_total, causal != 0); out[3 * m + 1] = (i64)(r0 + t); out[3 * m + 2] = (i64)j;
            ++m;
        }
    return m;
}

// last pass of a rotate-and-add step: rows (item, limb, slice, live)
unsigned wm_rotate_add_slices(size_t n) { return RotateAddMap::slices(n); }
int wm_rotate_add_staged(size_t n) { return RotateAddMap::staged(n); }
u64 wm_rotate_add_grid(size_t n_polys, unsigned slices) { return RotateAddMap::grid(n_polys, slices); }
void wm_rotate_add_decode(unsigned n_ids, unsigned slices, size_t n_polys, unsigned n_data_limbs, i64* out) {
    for (unsigned id = 0; id < n_ids; ++id) {
        const RotateAddWork w = RotateAddMap::decode(id, slices, n_polys, n_data_limbs);
        i64* o = out + 4 * (size_t)id;
        o[0] = (i64)w.item; o[1] = w.limb; o[2] = w.slice; o[3] = w.live;
    }
}

// items in chunks: the plan -> grid (threads, log2_chunks, ok through the pointers); the same with the chunk count given (the encoders' first kernels);
// rows (outer, lane), one per THREAD of every id, in id-major order
u64 wm_item_chunk_plan(size_t outer, unsigned lanes_per_outer, unsigned max_threads, unsigned* threads, unsigned* log2_chunks, int* ok) {
    const ItemChunkPlan p = ItemChunkMap::plan(outer, lanes_per_outer, max_threads);
    *threads = p.threads; *log2_chunks = p.log2_chunks; *ok = p.ok;
    return p.grid;
}
u64 wm_item_chunk_fixed(size_t outer, unsigned threads, unsigned log2_chunks, int* ok) {
    const ItemChunkPlan p = ItemChunkMap::fixed(outer, threads, log2_chunks);
    *ok = p.ok;
    return p.grid;
}
void wm_item_chunk_lanes(unsigned n_ids, unsigned log2_chunks, unsigned threads, i64* out) {
    for (unsigned id = 0; id < n_ids; ++id) {
        const ItemChunkWork w = ItemChunkMap::decode(id, log2_chunks);
        for (unsigned t = 0; t < threads; ++t, out += 2) { out[0] = w.outer; out[1] = ItemChunkMap::lane<size_t>(w.chunk, threads, t); }
    }
}

// batched transforms: rows (first word / N, limb, sub-block)
void wm_transform_decode(unsigned n_ids, int n_sub, int n_limbs, int n_active, unsigned long long active_map, i64* out) {
    const Tables tb{n_sub, n_limbs, n_active, active_map};
    for (unsigned id = 0; id < n_ids; ++id) {
        const TransformBlock b = transform_block(tb, id);
        out[3 * id] = (i64)b.p; out[3 * id + 1] = b.limb; out[3 * id + 2] = (i64)b.sub;
    }
}

// Galois source positions of all N output positions; 0, or -1 for a ring degree not compiled here
int wm_galois_src_pos(int log2n, unsigned g, i64* out) {
    switch (log2n) {
        case 8: src_pos_all<8>(g, out); return 0;
        case 9: src_pos_all<9>(g, out); return 0;
        case 10: src_pos_all<10>(g, out); return 0;
        case 11: src_pos_all<11>(g, out); return 0;
        case 12: src_pos_all<12>(g, out); return 0;
        case 13: src_pos_all<13>(g, out); return 0;
        case 14: src_pos_all<14>(g, out); return 0;
        case 15: src_pos_all<15>(g, out); return 0;
        case 16: src_pos_all<16>(g, out); return 0;
        default: return -1;
    }
}

// g^-1 mod 2N as the launchers of the coefficient-domain rotations take it; for every odd g < two_n at once: out[(g - 1) / 2]
unsigned wm_galois_inverse(unsigned g, unsigned two_n) { return galois_inverse(g, two_n); }
void wm_galois_inverse_all(unsigned two_n, i64* out) {
    for (unsigned g = 1; g < two_n; g += 2) out[g >> 1] = galois_inverse(g, two_n);
}

}  // extern "C"
