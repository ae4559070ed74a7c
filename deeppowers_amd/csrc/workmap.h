// workmap.h - where a workgroup works: the decode of a workgroup id into its work item, and the grid that decode expects, once per kernel family.
// No HIP: kernels, launchers (launch_impl.h, cabi_*.hip) and tools/emulate_workmap.cpp read the same text, so every layout is enumerated on the
// CPU (tests/test_work_maps_cpu.py: coverage, dead ids, locality) before it runs on a GPU.  A layout change starts in that test.
// Each decode keeps the arithmetic and the statement order its kernels had before it moved here (a dead id leaves early where they returned early, and
// carries a flag where they computed everything first): hipcc's register counts follow that order - MEASUREMENTS.md, "One work map per kernel family".
#pragma once
#include <stddef.h>

#include "ntt_core.h"

namespace dpfhe {

// ------------------------------------------------------------------------------------------------
// The "deal to 8 XCDs" layout.  The hardware deals workgroup ids to the 8 XCDs round-robin, so ids that are equal modulo 8 run on the same XCD
// (behind the same L2), and ids adjacent above that (id >> 3) run there at about the same time.  `count` outer items x `group` inner items:
// the `group` workgroups of an outer item get ids equal modulo 8 and consecutive above that - whatever they share comes from HBM once and
// is an L2 hit for the rest.  Outer items are dealt in rounds of 8; ids of a last, partly filled round decode to outer >= count and return.
// ------------------------------------------------------------------------------------------------
struct XcdSlot { unsigned outer, inner; };
struct xcd_deal {
    static DPF_HD unsigned xcd(unsigned id) { return id & 7u; }                              // where the id runs
    static DPF_HD unsigned slot(unsigned id) { return id >> 3; }                             // ... and when, among the ids of that XCD
    static DPF_HD unsigned outer(unsigned round, unsigned xcd) { return round * 8u + xcd; }  // outer item of slot `round * group + inner` of an XCD
    static DPF_HD XcdSlot decode(unsigned id, unsigned group) {
        const unsigned q = slot(id);
        return XcdSlot{outer(q / group, xcd(id)), q % group};
    }
    static DPF_HD size_t grid(size_t count, size_t group) { return ((count + 7) / 8) * 8 * group; }
};

// ------------------------------------------------------------------------------------------------
// Key switching (kernels.h relin_kernel, relin_shared_kernel): `blocks` = items x La workgroups, La = the limbs the launch works on.  Three layouts:
//   plain      id = item La + limb (items that share ONE key: an XCD only ever touches the key tiles of its own limbs);
//   grouped    `key_group` consecutive items share a key: outer = (group of items, limb), inner = item in the group - the key tiles of a limb
//              come from HBM once per group;
//   key-major  eight keys or more: outer = key, inner = (limb, item in the group), limb-major - ALL workgroups of a key on one XCD, so the items'
//              digits (read by every limb's workgroup) and the key tiles (read by every item's workgroup) both come from HBM once.
// The layout travels in the kernel argument n_outer: 0 = plain, otherwise the number of outer items of the grouped layout, kRelinRotMajor set for key-major.
// ------------------------------------------------------------------------------------------------
constexpr unsigned kRelinRotMajor = 0x80000000u;
struct RelinWork {
    size_t item;
    int limb_index;   // index into the launch's limbs (the limb itself, or through DevTables::active_map for one class of a mixed context)
    bool live;
};
struct RelinPlan { unsigned n_outer; size_t grid; };
struct RelinMap {
    static DPF_HD RelinWork decode(unsigned id, unsigned n_outer, unsigned key_group, unsigned La) {
        const RelinWork dead{0, 0, false};
        if (n_outer & kRelinRotMajor) {
            const unsigned n_keys = (n_outer & ~kRelinRotMajor) / La;
            const XcdSlot s = xcd_deal::decode(id, La * key_group);   // (key, limb-major index inside the key)
            if (s.outer >= n_keys) return dead;
            return RelinWork{(size_t)s.outer * key_group + s.inner % key_group, (int)(s.inner / key_group), true};
        }
        if (n_outer) {
            const XcdSlot s = xcd_deal::decode(id, key_group);        // ((group of items, limb), item in the group)
            if (s.outer >= n_outer) return dead;
            return RelinWork{(size_t)(s.outer / La) * key_group + s.inner, (int)(s.outer % La), true};
        }
        return RelinWork{id / La, (int)(id % La), true};
    }
    // blocks <= 2^31 - 1 (the callers' kMaxGrid check comes first); key_group 0 means 1
    static DPF_HD RelinPlan plan(size_t blocks, unsigned La, size_t key_stride, unsigned key_group) {
        const unsigned kg = key_group ? key_group : 1u;
        // (items with a key each and NO sharing - one token's rotations - take the XCD layouts too: all limbs of an item on one XCD, so that its digits cross
        //  the fabric once, not once per XCD - profiles/r06_giant_traffic.txt, shape (15, 1).)  Whole groups only.
        RelinPlan p;
        p.n_outer = ((kg > 1 || key_stride != 0) && blocks % ((size_t)kg * La) == 0) ? (unsigned)(blocks / kg) : 0u;
        p.grid = p.n_outer ? xcd_deal::grid(p.n_outer, kg) : blocks;
        if (p.n_outer && p.n_outer / La >= 8u) {
            p.grid = xcd_deal::grid(p.n_outer / La, (size_t)La * kg);
            p.n_outer |= kRelinRotMajor;
        }
        return p;
    }
};

// ------------------------------------------------------------------------------------------------
// Hoisted rotations (kernels.h hoisted_ks_kernel: split, one workgroup per key component; hoisted_ks2_kernel: merged): outer = key tile =
// (rotation, limb[, component]), inner = token - the n_items workgroups that read one key tile are neighbours on one XCD.
// ------------------------------------------------------------------------------------------------
struct HoistedWork {
    size_t rot;
    int limb_index, comp;
    unsigned token;
    bool live;
};
struct HoistedPlan { unsigned tiles, blocks; };
struct HoistedMap {
    template <bool MERGED>
    static DPF_HD HoistedWork decode(unsigned id, unsigned n_items, unsigned n_tiles, unsigned La) {
        const XcdSlot s = xcd_deal::decode(id, n_items);
        if (s.outer >= n_tiles) return HoistedWork{0, 0, 0, 0, false};
        const unsigned rl = MERGED ? s.outer : s.outer >> 1;   // (rotation, limb)
        return HoistedWork{(size_t)(rl / La), (int)(rl % La), MERGED ? 0 : (int)(s.outer & 1u), s.inner, true};
    }
    static DPF_HD HoistedPlan plan(size_t count, unsigned La, size_t n_items, bool merged) {
        HoistedPlan p;
        p.tiles = (unsigned)(count * (size_t)La) * (merged ? 1u : 2u);
        p.blocks = (unsigned)xcd_deal::grid(p.tiles, n_items);
        return p;
    }
};

// ------------------------------------------------------------------------------------------------
// Matrix-vector products (kernels_linalg.h matvec_kernel, matvec_multi_kernel, matvec_fold_kernel): outer = slab = (limb, chunk of words), inner =
// (row tile, group of right-hand sides), group fastest.  The G workgroups of a row tile read the same W tile and the R workgroups of a group the
// same x tile at about the same time, on XCD slab % 8: each is fetched from HBM once.
// ------------------------------------------------------------------------------------------------
struct MatvecWork {
    int limb, chunk;
    unsigned row_tile, group;
    bool live;
};
struct MatvecMap {
    static DPF_HD MatvecWork decode(unsigned id, unsigned n_limbs, unsigned chunks, unsigned row_tiles, unsigned n_groups) {
        const unsigned q = xcd_deal::slot(id), group = q % n_groups, rt = (q / n_groups) % row_tiles;
        const unsigned slab = xcd_deal::outer(q / (n_groups * row_tiles), xcd_deal::xcd(id));
        return MatvecWork{(int)(slab / chunks), (int)(slab % chunks), rt, group, slab < n_limbs * chunks};
    }
    static DPF_HD size_t grid(size_t n_limbs, size_t chunks, size_t row_tiles, size_t n_groups) { return xcd_deal::grid(n_limbs * chunks, row_tiles * n_groups); }
};

// ------------------------------------------------------------------------------------------------
// The coefficient-domain rotations gather word k of sigma_g(a) from position k g^-1 mod 2N (kernels_rotate.h): their launchers invert the element here.
// g^-1 mod 2N by Newton iteration (g odd): x <- x (2 - g x) doubles the correct low bits, 1 -> 32 in five steps.  Host only.
// ------------------------------------------------------------------------------------------------
inline unsigned galois_inverse(unsigned g, unsigned two_n) {
    unsigned inv = 1;
    for (int i = 0; i < 5; ++i) inv *= 2u - g * inv;
    return inv & (two_n - 1u);
}

// ------------------------------------------------------------------------------------------------
// Baby steps of the double-hoisted products (kernels_rotate.h hoisted_qp_stream_kernel, hoisted_qp_upfront_kernel): a workgroup is 256 threads x
// `pairs` 16-byte pairs = one segment of one (rotation, limb, token).  outer = combo = (limb, SOURCE segment), inner = (rotation group, rotation in
// the group, token): XCD combo % 8 gets, one block of kQpRotGroup rotations x n_items tokens at a time, all workgroups of one combo - every key
// segment is fetched from HBM once for its tokens and every digit segment once for its 16 rotations.
// ------------------------------------------------------------------------------------------------
constexpr int kQpPairs = 2;          // 16-byte pairs per thread of the stream kernel: segment = 512 pairs = 1024 words
constexpr int kQpRotGroup = 16;      // rotations that share a digit segment in one XCD block
struct QpGeo {
    int n1;                            // log2 of the pairs per polynomial
    unsigned half, n, seg_pairs, nseg, tbits;   // pairs and words per polynomial, pairs per segment, segments per polynomial and their log2
};
struct QpWork {
    int limb;
    unsigned sseg, rot, token;
    bool live;
};
struct QpPair {
    unsigned out, src;   // pair written (lane-contiguous inside the output segment), pair gathered (inside source segment sseg)
    bool swap, ok;       // the pair's two words arrive swapped; out is inside the polynomial (rings below one segment)
};
struct QpMap {
    static DPF_HD QpGeo geo(int log2n, unsigned pairs) {
        QpGeo g;
        g.n1 = log2n - 1;
        g.half = 1u << g.n1;
        g.n = 2u << g.n1;
        g.seg_pairs = 256u * pairs;
        g.nseg = g.half > g.seg_pairs ? g.half / g.seg_pairs : 1u;
        g.tbits = 31u - (unsigned)__builtin_clz(g.nseg);
        return g;
    }
    static DPF_HD unsigned rot_groups(unsigned n_rot) { return (n_rot + kQpRotGroup - 1) / kQpRotGroup; }
    static DPF_HD QpWork decode(unsigned id, const QpGeo& g, unsigned n_limbs, unsigned n_rot, unsigned n_items) {
        const unsigned n_rg = rot_groups(n_rot), bs = (unsigned)kQpRotGroup * n_items;
        const unsigned q = xcd_deal::slot(id), within = q % bs, t1 = q / bs, rg = t1 % n_rg, combo = xcd_deal::outer(t1 / n_rg, xcd_deal::xcd(id));
        const unsigned rot = rg * kQpRotGroup + within / n_items, token = within % n_items;
        return QpWork{(int)(combo % n_limbs), combo / n_limbs, rot, token, combo < n_limbs * g.nseg && rot < n_rot};
    }
    // 8 XCDs x blocks of (16 rotations x n_items) x rotation groups x ceil(L nseg / 8)
    static DPF_HD size_t grid(int log2n, size_t n_limbs, size_t n_rot, size_t n_items, unsigned pairs = kQpPairs) {
        return xcd_deal::grid(n_limbs * geo(log2n, pairs).nseg, (n_rot + kQpRotGroup - 1) / kQpRotGroup * (size_t)kQpRotGroup * n_items);
    }
    // sigma_g in forward-output order maps every aligned pair ONTO an aligned pair (swapped or not) and every aligned segment onto an aligned segment:
    //   pair m -> pair m' = brv((c - 1) / 2),  c = g (2 brv(m) + 1) mod 2N reduced mod N,  words swapped iff that product is >= N   (brv over log2 N - 1 bits).
    // The workgroup of SOURCE segment sseg writes the output segment oseg with 2 brv(oseg) + 1 = g^-1 (2 brv(sseg) + 1) mod 2 nseg; `lane` = pair inside it.
    static DPF_HD unsigned brv(unsigned x, int bits) { return bits ? (brev32(x) >> (32 - bits)) : 0u; }
    static DPF_HD QpPair pair_map(unsigned g, unsigned sseg, unsigned lane, const QpGeo& geo) {
        unsigned ginv = g;
        for (int i = 0; i < 4; ++i) ginv *= 2u - g * ginv;                  // g^-1 mod 2^32
        const unsigned uo = (ginv * (2u * brv(sseg, (int)geo.tbits) + 1u)) & (2u * geo.nseg - 1u);
        const unsigned oseg = brv((uo - 1u) >> 1, (int)geo.tbits);
        QpPair p;
        p.out = oseg * geo.seg_pairs + lane;
        p.ok = p.out < geo.half;
        const unsigned cf = (g * (2u * brv(p.out, geo.n1) + 1u)) & (2u * geo.n - 1u);
        p.swap = cf >= geo.n;
        p.src = brv(((cf & (geo.n - 1u)) - 1u) >> 1, geo.n1);
        return p;
    }
};

// ------------------------------------------------------------------------------------------------
// The streaming kernels take their work in 512-word chunks of a residue polynomial: 256 threads x one 16-byte pair (the `chunks` argument of each;
// a thread owns words chunk * 512 + 2 tid and the next).  Rings below N = 512 have one partial chunk, whose upper threads idle.
// id = (poly * n_limbs + limb) * chunks + chunk.
// ------------------------------------------------------------------------------------------------
constexpr int chunks_of(size_t n) { return (int)((n + 511) / 512); }
struct ChunkWork {
    int chunk, limb;
    size_t poly;
};
template <class Limbs>   // (the limb count as the kernel holds it: the divisions run in its type)
DPF_HD ChunkWork chunk_work(unsigned id, int chunks, Limbs n_limbs) {
    return ChunkWork{(int)(id % chunks), (int)((id / chunks) % n_limbs), (size_t)(id / chunks / n_limbs)};
}
// the grid of a last pass that drops the last data prime as well (relin_rescale_kernel, relin_lincomb_rescale_kernel): chunk_work over the 2 polynomials of
// every item and the Ld - 1 kept limbs
constexpr size_t relin_rescale_grid(size_t batch, size_t n_data_limbs, size_t n) { return batch * 2 * (n_data_limbs - 1) * (size_t)chunks_of(n); }
// the grid of a sum of tensor products (kernels_mul.h tensor3_sum_kernel): chunk_work with the GROUP in the polynomial's place - a workgroup owns one chunk of one
// limb of all three output rows of its group
constexpr size_t mul_sum_grid(size_t groups, size_t n_limbs, size_t n) { return groups * n_limbs * (size_t)chunks_of(n); }
// the grid of the complement products (kernels_mul.h tensor3_complement_kernel): the same map - a workgroup owns one chunk of one limb of its group's factor and of
// all three rows of every product of the group, however many items the group has and whether the self product is among them
constexpr size_t mul_complement_grid(size_t groups, size_t n_limbs, size_t n) { return groups * n_limbs * (size_t)chunks_of(n); }

// ------------------------------------------------------------------------------------------------
// All pairs of A resident operands and B streamed ones (kernels_mul.h tensor3_outer_kernel): outer = slab = (limb, 512-word chunk), inner = tile of
// kMulOuterTile resident operands.  A workgroup keeps its tile's chunk in registers and walks the streamed operands' chunk; the `tiles` workgroups of a slab read
// the SAME streamed rows, so they share ONE XCD, consecutive in its order: the rows come from HBM once and are L2 hits for the other tiles.  Ids of a last,
// partly filled round of slabs are dead.  A tile may be ragged (rows past a_count), and under the causal flag a tile walks the streamed operands up to its
// last row's only: `keys` and `writes` are that predicate, once, for the kernel, the launcher's callers and the enumeration on the CPU.
// ------------------------------------------------------------------------------------------------
constexpr int kMulOuterTile = 4;
struct MulOuterWork {
    int limb, chunk;
    size_t tile;
    bool live;
};
struct MulOuterMap {
    static DPF_HD size_t tiles(size_t a_count) { return (a_count + kMulOuterTile - 1) / kMulOuterTile; }
    static DPF_HD MulOuterWork decode(unsigned id, unsigned tiles, unsigned n_limbs, unsigned chunks) {
        const XcdSlot s = xcd_deal::decode(id, tiles);
        if (s.outer >= n_limbs * chunks) return MulOuterWork{0, 0, 0, false};
        return MulOuterWork{(int)(s.outer / chunks), (int)(s.outer % chunks), (size_t)s.inner, true};
    }
    static DPF_HD size_t grid(size_t a_count, size_t n_limbs, size_t n) { return xcd_deal::grid(n_limbs * (size_t)chunks_of(n), tiles(a_count)); }
    // the streamed operands a tile whose first row is local row r0 walks: all b_count, or under the causal flag those with b_off + j <= the GLOBAL index of the
    // tile's last row (a_off, b_off: where the launch's ranges start among all operands; a block above the diagonal walks none)
    static DPF_HD size_t keys(size_t r0, size_t a_count, size_t b_count, size_t a_off, size_t b_off, bool causal) {
        if (!causal) return b_count;
        const size_t rows = a_count - r0 < (size_t)kMulOuterTile ? a_count - r0 : (size_t)kMulOuterTile, last = a_off + r0 + rows - 1;
        if (last < b_off) return 0;
        return last - b_off + 1 < b_count ? last - b_off + 1 : b_count;
    }
    // whether the pair (local row i, local streamed j) is written
    static DPF_HD bool writes(size_t i, size_t j, size_t a_off, size_t b_off, bool causal) { return !causal || b_off + j <= a_off + i; }
    // ... and where: item i B + j of the full form (b_total = B streamed operands in all), item i (i + 1) / 2 + j of the causal one, in GLOBAL indices
    static DPF_HD size_t item(size_t i, size_t j, size_t a_off, size_t b_off, size_t b_total, bool causal) {
        const size_t gi = a_off + i, gj = b_off + j;
        return causal ? gi * (gi + 1) / 2 + gj : gi * b_total + gj;
    }
};

// ------------------------------------------------------------------------------------------------
// The last pass of a rotate-and-add step (kernels_rotate.h rotate_add_pass_kernel): outer = (item, data limb), inner = slice of that residue polynomial's
// chunks.  A workgroup writes its slice of BOTH components; component 0 gathers sigma_g(c0) from anywhere in the polynomial, so the `slices`
// workgroups of a polynomial share ONE XCD: staged (the polynomial fits 64 KiB of LDS, N <= 8192) each of them reads all of c0 - from HBM once, L2 hits
// for the rest -, at most 8 of them; unstaged the gathers of all chunks go to that XCD's L2.  slices divides chunks (powers of two).
// ------------------------------------------------------------------------------------------------
constexpr int kRotateAddStagedMaxN = 8192;
struct RotateAddWork {
    size_t item;
    int limb;
    unsigned slice;
    bool live;
};
struct RotateAddMap {
    static DPF_HD bool staged(size_t n) { return n <= (size_t)kRotateAddStagedMaxN; }
    static DPF_HD unsigned slices(size_t n) {
        const unsigned chunks = (unsigned)chunks_of(n);
        return staged(n) && chunks > 8u ? 8u : chunks;
    }
    static DPF_HD RotateAddWork decode(unsigned id, unsigned slices, size_t n_polys, unsigned n_data_limbs) {
        const XcdSlot s = xcd_deal::decode(id, slices);
        if (s.outer >= n_polys) return RotateAddWork{0, 0, 0, false};
        return RotateAddWork{(size_t)(s.outer / n_data_limbs), (int)(s.outer % n_data_limbs), s.inner, true};
    }
    static DPF_HD size_t grid(size_t n_polys, unsigned slices) { return xcd_deal::grid(n_polys, slices); }   // n_polys = items x data limbs
};

// ------------------------------------------------------------------------------------------------
// Items in chunks (the byte-stream and encoding families: k_expand, k_noise, k_plain_add, k_compact, k_encode, k_cencode .hip): `outer` items (an item, or an
// (item, limb)) of `lanes` lanes each, a workgroup = one chunk of `threads` lanes.  id = (outer << log2_chunks) + chunk; thread t of the chunk is lane
// chunk * threads + t of its outer item.  Powers of two throughout: threads << log2_chunks is the lane count exactly, so no id and no thread is dead.
// `plan` is the launch AND the "too large for one launch" bound of the entries (constexpr: a kernel with constant geometry takes its log2_chunks from it);
// the encoders' first kernels choose their chunk themselves (a workgroup walks it): `fixed`, and call `chunk` and `outer` where their statements had the two.
// ------------------------------------------------------------------------------------------------
struct ItemChunkWork { unsigned outer, chunk; };
struct ItemChunkPlan { unsigned threads, log2_chunks; size_t grid; bool ok; };   // ok: an item at least, no overflow of the shift, at most 2^31 - 1 workgroups
struct ItemChunkMap {
    static DPF_HD unsigned chunk(unsigned id, unsigned log2_chunks) { return id & ((1u << log2_chunks) - 1u); }
    static DPF_HD unsigned outer(unsigned id, unsigned log2_chunks) { return id >> log2_chunks; }
    static DPF_HD ItemChunkWork decode(unsigned id, unsigned log2_chunks) {
        const unsigned c = chunk(id, log2_chunks);
        return ItemChunkWork{outer(id, log2_chunks), c};
    }
    template <class I = unsigned>   // (the index in the type the kernel computes its offsets in)
    static DPF_HD I lane(unsigned chunk, unsigned threads, unsigned tid) { return (I)chunk * threads + tid; }
    static constexpr DPF_HD ItemChunkPlan fixed(size_t outer, unsigned threads, unsigned log2_chunks) {
        ItemChunkPlan p{threads, log2_chunks, outer << log2_chunks, false};
        p.ok = outer != 0 && (p.grid >> log2_chunks) == outer && p.grid <= (size_t)0x7fffffffu;
        return p;
    }
    static constexpr DPF_HD ItemChunkPlan plan(size_t outer, unsigned lanes_per_outer, unsigned max_threads) {
        const unsigned threads = lanes_per_outer < max_threads ? lanes_per_outer : max_threads;
        unsigned log2_chunks = 0;
        while ((threads << log2_chunks) < lanes_per_outer) ++log2_chunks;
        return fixed(outer, threads, log2_chunks);
    }
    // one lane per pair of coefficients of a residue polynomial (16 bytes of each limb row), at most 256 lanes per workgroup (log2n >= 8: at least two waves)
    static DPF_HD ItemChunkPlan pairs(size_t items, unsigned log2n) { return plan(items, 1u << (log2n - 1), 256u); }
};

}  // namespace dpfhe
