// The contract between the fused edge-chain kernels and the host code that feeds them, stated ONCE per family: how a weight image is
// chunked, how large it is, where a sub-image starts, how many blocks a launch has, where a section's ReLU-mask words sit, and which
// width sets have an instantiation.  Plain constexpr functions and constant structs: the kernels read them as template-time
// constants, the packers / planners / launchers with run-time widths, and the static_asserts at the end pin them for the shipped
// width sets.  Nothing here is a run-time object and nothing here is passed to a kernel.
//   fp32 / split family: edge_chain.hip (edge_chain_kernel, edge_chain_bwd_kernel, pack_edge_chain, pack_edge_chain_bwd)
//   bf16 family:         edge_chain_bf16.hip, edge_chain_bf16_bwd.hip
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace mpnhip {

// ---- both families: widths are padded to 32-feature tiles ---------------------------------------------------------------------
constexpr int chain_tiles(int width) { return (width + 31) / 32; }
constexpr int pad32(int width) { return 32 * chain_tiles(width); }
constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int cmin(int a, int b) { return a < b ? a : b; }

// ReLU-mask words of one lane of a 32-edge wave tile: two 32-feature tiles per 32-bit word, one word range per section
// H1 | e' | HC | HF | M; word w of wave tile q sits at mask[(q * nw + w) * 64 + lane].  Arguments are TILE counts.
struct ChainMaskSections { int h1, e, hc, hf, m, nw; };
constexpr int chain_pair_words(int tiles) { return (tiles + 1) / 2; }
constexpr ChainMaskSections chain_mask_sections(int t1, int t2, int tc, int tf, int td) {
    const int e = chain_pair_words(t1), hc = e + chain_pair_words(t2), hf = hc + chain_pair_words(tc), m = hf + chain_pair_words(tf);
    return {0, e, hc, hf, m, m + chain_pair_words(td)};
}
// the same for a kernel's template-time tile counts, as plain constants (a constexpr struct local to a kernel is an object in its frame)
template <int T1, int T2, int TC, int TF, int TD>
struct ChainMaskWords {
    static constexpr int H1 = chain_mask_sections(T1, T2, TC, TF, TD).h1, E = chain_mask_sections(T1, T2, TC, TF, TD).e,
                         HC = chain_mask_sections(T1, T2, TC, TF, TD).hc, HF = chain_mask_sections(T1, T2, TC, TF, TD).hf,
                         M = chain_mask_sections(T1, T2, TC, TF, TD).m, NW = chain_mask_sections(T1, T2, TC, TF, TD).nw;
};
// first word of section i (0 H1, 1 e', 2 HC, 3 HF, 4 M)
constexpr int chain_mask_section_word(const ChainMaskSections& s, int i) { return i == 0 ? s.h1 : i == 1 ? s.e : i == 2 ? s.hc : i == 3 ? s.hf : s.m; }

// ================================================== fp32 / split family ==========================================================
constexpr int CHAIN_HC = 32;   // the classifier's hidden width as the kernels see it: one tile (hc <= 32)

// ---- launch geometry: blocks of 4 waves x 32 edges; each of the three direction groups (out | in | self loops) starts on a block
// boundary, hence the spare blocks
struct ChainGeom {
    static constexpr int EPB_LOG2 = 7, EPB = 1 << EPB_LOG2, WAVES = EPB / 32, THREADS = 64 * WAVES, SPARE = 3;
};
constexpr int chain_group_blocks(int edges) { return (edges + ChainGeom::EPB - 1) >> ChainGeom::EPB_LOG2; }   // blocks of one direction group
constexpr unsigned chain_blocks(int64_t E) { return (unsigned)((E + ChainGeom::EPB - 1) / ChainGeom::EPB + ChainGeom::SPARE); }

constexpr int chain_mask_words(int he, int de, int hn, int dn) {
    return chain_mask_sections(chain_tiles(he), chain_tiles(de), chain_tiles(CHAIN_HC), chain_tiles(hn), chain_tiles(dn)).nw;
}
// one step's mask buffer: every wave tile of the launch (spare blocks included) holds nw x 64 words
constexpr size_t chain_mask_ints(int64_t E, int he, int de, int hn, int dn) {
    return (size_t)chain_blocks(E) * ChainGeom::WAVES * 64 * (size_t)chain_mask_words(he, de, hn, dn);
}

// ---- images.  An image (or any whole-row / whole-block part of one) of `elems` padded elements takes `elems` floats as fp32 and
// elems * 6 bytes = 3/2 as many floats as a three-piece bf16 split image; the split layout keeps the fp32 image's chunk schedule
// with every offset and size scaled alike (edge_chain.hip, split8)
struct ChainScale { static constexpr int DEN = 2; static constexpr int num(bool split) { return split ? 3 : 2; } };   // floats per element = num / DEN
constexpr int64_t chain_floats(int64_t elems, bool split) { return elems * ChainScale::num(split) / ChainScale::DEN; }
constexpr int chain_f4(int elems, bool split) { return elems / 4 * ChainScale::num(split) / ChainScale::DEN; }   // the same as a float4 count (LDS-DMA pieces)
// floats a buffer must have to hold the image in either form
constexpr size_t chain_image_capacity(size_t elems) { return (size_t)chain_floats((int64_t)elems, true); }
// a [k][n] image is streamed in chunks of whole k rows: offset of row k of an image with ncols padded columns
constexpr int64_t chain_row_off(int64_t k, int ncols, bool split) { return chain_floats(k * ncols, split); }

// Forward chunk schedule (edge_chain_kernel).  Images: w1T [K1][HE], w2T [HE][DE], wc1T [DE][CHAIN_HC], wf2T [HN][DN] as whole-row
// chunks; flow layer 0 as ONE IMAGE [DE][<= NC4] PER BLOCK of NC4 output features (the kernel streams whole blocks)
struct ChainFwd {
    static constexpr int KC1 = 16;   // phase 1: [16 k][HE] of w1T (k1a / k1b / the Q0 row offset are multiples of it)
    static constexpr int KC2 = 64;   // phase 2: [<= 64 k][DE] of w2T
    static constexpr int NC4 = 64;   // phase 4: one block image [DE k][<= 64 n] of wf1T
    static constexpr int KC5 = 32;   // phase 5: [32 k][DN] of wf2T
};
constexpr int chain_nchunks(int total, int per_chunk) { return (total + per_chunk - 1) / per_chunk; }
constexpr int chain_chunk_len(int total, int per_chunk, int i) { return total - i * per_chunk < per_chunk ? total - i * per_chunk : per_chunk; }   // rows / columns of chunk i
constexpr int chain_wf1_blocks(int HN) { return chain_nchunks(HN, ChainFwd::NC4); }
constexpr int chain_wf1_block_cols(int HN, int i) { return chain_chunk_len(HN, ChainFwd::NC4, i); }
constexpr int64_t chain_wf1_block_off(int DE, int i, bool split) { return chain_floats((int64_t)DE * ChainFwd::NC4 * i, split); }

// Backward chunk schedule (edge_chain_bwd_kernel).  Images in the weights' native [n][k] orientation: wf2 [DN][HN], wfe [HN][DE],
// wc1 [CHAIN_HC][DE], w2 [DE][HE] as whole-row chunks; the e-part columns of edge layer 0 as ONE IMAGE [HE][ncol] PER PASS of <= NC6
// padded columns of [e0 | e_{s-1}] (KEp of them: each half padded to DE)
struct ChainBwd {
    static constexpr int NR2 = 16;   // B2: [16 n][HN] of wf2
    static constexpr int NR3 = 64;   // B3: [<= 64 n][DE] of wfe
    static constexpr int NR5 = 16;   // B5: [16 n][HE] of w2
    static constexpr int NR6 = 64;   // B6: [<= 64 n][ncol] of one pass image of w1e
    static constexpr int NC6 = 64;   // B6: columns per pass
};
constexpr int chain_w1e_cols(int KEp) { return cmin(KEp, ChainBwd::NC6); }                          // columns of every pass image
constexpr int chain_w1e_passes(int KEp) { return KEp / ChainBwd::NC6 > 0 ? KEp / ChainBwd::NC6 : 1; }
// row `row` of pass image `pass` (ncol = chain_w1e_cols)
constexpr int64_t chain_w1e_off(int64_t pass, int HE, int row, int ncol, bool split) { return chain_floats((pass * HE + row) * ncol, split); }
// padded column col0 of [e0 | e_{s-1}] lives in pass col0 / NC6 at column col0 % NC6
constexpr int chain_w1e_pass_of(int col0) { return col0 / ChainBwd::NC6; }
constexpr int chain_w1e_col_in_pass(int col0) { return col0 % ChainBwd::NC6; }
// EdgeChainBwdArgs::skip_e0 leaves out whole passes: each half of [e0 | e_{s-1}] must be exactly one (32 < de <= 64)
constexpr bool chain_e0_half_is_one_pass(int DE) { return DE == ChainBwd::NC6; }

// floats of the largest chunk buffer either kernel needs: whole 1 KiB LDS-DMA pieces (split images: exactly the largest chunk)
constexpr int chain_chunk_buffer_floats(int n4_max, bool split) { return split ? 4 * n4_max : 1024 * ((n4_max + 255) / 256); }

// ---- supported width sets: the dispatch table of launch_edge_chain / launch_edge_chain_bwd.  exact_form: widths that are all
// multiples of 32 (hc == 32) have an instantiation of their own without load / store masks
struct ChainVariant { int name, t1, t2, tf, td; bool exact_form; };
constexpr ChainVariant CHAIN_VARIANTS[] = {
    {128, 10, 2, 7, 4, true},    // BASELINE.json 128-d: he 320, de 64, hn 224, dn 128
    {64, 5, 1, 4, 2, false},     // 64-d
    {32, 3, 1, 2, 1, false},     // the reference's shipped 32-d dims: 80 / 16 / 56 / 32
};
constexpr int CHAIN_NVARIANTS = (int)(sizeof(CHAIN_VARIANTS) / sizeof(CHAIN_VARIANTS[0]));
// index into CHAIN_VARIANTS or -1
constexpr int chain_variant(int he, int de, int hn, int dn) {
    for (int i = 0; i < CHAIN_NVARIANTS; ++i) {
        const ChainVariant& v = CHAIN_VARIANTS[i];
        if (chain_tiles(he) == v.t1 && chain_tiles(de) == v.t2 && chain_tiles(hn) == v.tf && chain_tiles(dn) == v.td) return i;
    }
    return -1;
}
constexpr bool chain_widths_exact(int he, int de, int hn, int dn, int hc) {
    return he % 32 == 0 && de % 32 == 0 && hn % 32 == 0 && dn % 32 == 0 && hc == CHAIN_HC;
}
template <int T1_, int T2_, int TF_, int TD_, bool EXACT_, bool SP_>
struct ChainInst { static constexpr int T1 = T1_, T2 = T2_, TF = TF_, TD = TD_; static constexpr bool EXACT = EXACT_, SP = SP_; };
// calls f(ChainInst<...>{}) for the instantiation that serves these widths; false: no such width set
// (variant I's instantiations are named before the recursion: kernels are emitted in table order)
template <int I = 0, class F>
inline bool chain_dispatch(int variant, bool exact, bool split, F&& f) {
    if constexpr (I < CHAIN_NVARIANTS) {
        if (variant == I) {
            constexpr ChainVariant V = CHAIN_VARIANTS[I];
            constexpr bool EX = V.exact_form;   // (no exact form: `exact` selects the masked one again)
            if (split && exact) f(ChainInst<V.t1, V.t2, V.tf, V.td, EX, true>{});
            else if (split) f(ChainInst<V.t1, V.t2, V.tf, V.td, false, true>{});
            else if (exact) f(ChainInst<V.t1, V.t2, V.tf, V.td, EX, false>{});
            else f(ChainInst<V.t1, V.t2, V.tf, V.td, false, false>{});
            return true;
        }
        return chain_dispatch<I + 1>(variant, exact, split, f);
    } else {
        return false;
    }
}

// ====================================================== bf16 family ===============================================================
// ---- supported width sets and their launch geometry (forward and backward share both: the mask words are addressed by (block,
// wave, lane)).  exact_only: the masked form of the variant does not fit the register budget; waves: 8 = 256 edges per block, one
// block per CU; 4 = 128 edges, two blocks per CU; ct: hidden tiles per weight chunk
struct ChainBf16Variant { int name, t1, t2, tf, td, tc; bool exact_only, exact_form; int waves, ct; };
constexpr ChainBf16Variant CHAIN_BF16_VARIANTS[] = {
    {256, 20, 4, 14, 8, 2, true, true, 4, 1},    // BASELINE.json configs[4]
    {128, 10, 2, 7, 4, 1, false, true, 8, 2},
    {64, 5, 1, 4, 2, 1, false, false, 8, 2},
    {32, 3, 1, 2, 1, 1, false, false, 8, 2},
};
constexpr int CHAIN_BF16_NVARIANTS = (int)(sizeof(CHAIN_BF16_VARIANTS) / sizeof(CHAIN_BF16_VARIANTS[0]));
constexpr int chain_bf16_variant(int he, int de, int hn, int dn, int hc) {
    for (int i = 0; i < CHAIN_BF16_NVARIANTS; ++i) {
        const ChainBf16Variant& v = CHAIN_BF16_VARIANTS[i];
        if (chain_tiles(he) == v.t1 && chain_tiles(de) == v.t2 && chain_tiles(hn) == v.tf && chain_tiles(dn) == v.td && chain_tiles(hc) == v.tc)
            return i;
    }
    return -1;
}
// the widths launch_edge_chain_bf16 has an instantiation for (the exactness its 256-d form asks for does not include hc) ...
constexpr bool chain_bf16_fwd_widths_ok(int he, int de, int hn, int dn, int hc) {
    const int v = chain_bf16_variant(he, de, hn, dn, hc);
    return v >= 0 && (!CHAIN_BF16_VARIANTS[v].exact_only || (he % 32 == 0 && de % 32 == 0 && hn % 32 == 0 && dn % 32 == 0));
}
// ... and launch_edge_chain_bf16_bwd (the forward's plan asks this before it saves in the bf16-row form, so that a width the
// backward cannot take trains on the unfused path)
constexpr bool chain_bf16_bwd_widths_exact(int he, int de, int hn, int dn, int hc) {
    return he % 32 == 0 && de % 32 == 0 && hn % 32 == 0 && dn % 32 == 0 && hc % 32 == 0;
}
constexpr bool edge_chain_bf16_bwd_supported(int he, int de, int hn, int dn, int hc) {
    const int v = chain_bf16_variant(he, de, hn, dn, hc);
    return v >= 0 && (!CHAIN_BF16_VARIANTS[v].exact_only || chain_bf16_bwd_widths_exact(he, de, hn, dn, hc));
}
// edges per block / waves per block of the launch for these widths (unsupported widths: the 8-wave form's)
constexpr void chain_bf16_geometry(int he, int de, int hn, int dn, int hc, int* epb, int* nw) {
    const int v = chain_bf16_variant(he, de, hn, dn, hc);
    *nw = v >= 0 ? CHAIN_BF16_VARIANTS[v].waves : 8;
    *epb = 32 * *nw;
}
constexpr int CHAIN_BF16_SPARE = 3;   // the three direction groups start on block boundaries
constexpr unsigned chain_bf16_blocks(int64_t E, int epb) { return (unsigned)((E + epb - 1) / epb + CHAIN_BF16_SPARE); }
// wave tiles a per-wave-tile buffer is sized for, whatever the geometry: the 8-wave form's, with one block to spare
// (the 4-wave form's ((E + 127) / 128 + 3) * 4 is never more)
constexpr size_t chain_bf16_wave_tiles_max(int64_t E) { return (size_t)((E + 255) / 256 + 4) * 8; }

template <int T1_, int T2_, int TF_, int TD_, int TC_, bool EXACT_, int NW_, int CT_>
struct ChainBf16Inst { static constexpr int T1 = T1_, T2 = T2_, TF = TF_, TD = TD_, TC = TC_, NW = NW_, CT = CT_; static constexpr bool EXACT = EXACT_; };
// calls f(ChainBf16Inst<...>{}); false: no instantiation for these widths (`exact` as the calling launcher defines it)
template <int I = 0, class F>
inline bool chain_bf16_dispatch(int variant, bool exact, F&& f) {
    if constexpr (I < CHAIN_BF16_NVARIANTS) {
        if (variant == I) {
            constexpr ChainBf16Variant V = CHAIN_BF16_VARIANTS[I];
            // (no exact form: the first branch names the masked one again)
            if (V.exact_form && exact) f(ChainBf16Inst<V.t1, V.t2, V.tf, V.td, V.tc, V.exact_form, V.waves, V.ct>{});
            else if constexpr (!V.exact_only) f(ChainBf16Inst<V.t1, V.t2, V.tf, V.td, V.tc, false, V.waves, V.ct>{});
            else return false;
            return true;
        }
        return chain_bf16_dispatch<I + 1>(variant, exact, f);
    } else {
        return false;
    }
}

// mask words per lane of one 32-edge wave tile and the size of one step's mask buffer
constexpr int chain_bf16_mask_words(int he, int de, int hn, int dn, int hc) {
    return chain_mask_sections(chain_tiles(he), chain_tiles(de), chain_tiles(hc), chain_tiles(hn), chain_tiles(dn)).nw;
}
constexpr size_t chain_bf16_mask_ints(int64_t E, int he, int de, int hn, int dn, int hc) {
    return chain_bf16_wave_tiles_max(E) * 64 * (size_t)chain_bf16_mask_words(he, de, hn, dn, hc);
}
// bit of element r (0..15) of a tile with parity p inside its mask word
constexpr int chain_bf16_mask_bit(int p, int r) { return 8 * p + (r >> 1) + 16 * (r & 1); }

// ---- the description pinned against literals for the three shipped width sets (he, de, hn, dn) = (320, 64, 224, 128),
// (160, 32, 112, 64), (80, 16, 56, 32) ------------------------------------------------------------------------------------------
static_assert(chain_mask_words(320, 64, 224, 128) == 13 && chain_mask_words(160, 32, 112, 64) == 8 && chain_mask_words(80, 16, 56, 32) == 6,
              "mask words per lane (13 at 128-d is what the C ABI reports)");
static_assert(chain_mask_sections(10, 2, 1, 7, 4).e == 5 && chain_mask_sections(10, 2, 1, 7, 4).hc == 6 && chain_mask_sections(10, 2, 1, 7, 4).hf == 7 &&
              chain_mask_sections(10, 2, 1, 7, 4).m == 11, "mask sections at 128-d");
static_assert(chain_bf16_mask_words(640, 128, 448, 256, 64) == 24 && chain_bf16_mask_words(320, 64, 224, 128, 32) == 13, "bf16 mask words");
static_assert(chain_blocks(1) == 4 && chain_blocks(128) == 4 && chain_blocks(129) == 5 && chain_group_blocks(129) == 2, "blocks of 128 edges + 3");
static_assert(chain_mask_ints(50000, 320, 64, 224, 128) == (size_t)394 * 4 * 64 * 13, "mask buffer at cfg-B's edge count");
static_assert(chain_bf16_mask_ints(50000, 320, 64, 224, 128, 32) == (size_t)200 * 8 * 64 * 13, "bf16 mask buffer");
static_assert(chain_bf16_blocks(50000, 256) == 199 && chain_bf16_blocks(50000, 128) == 394, "bf16 launch blocks");
static_assert(chain_variant(320, 64, 224, 128) == 0 && chain_variant(160, 32, 112, 64) == 1 && chain_variant(80, 16, 56, 32) == 2 &&
              chain_variant(640, 128, 448, 256) == -1, "fp32 / split width sets");
static_assert(chain_bf16_variant(640, 128, 448, 256, 64) == 0 && chain_bf16_variant(80, 16, 56, 32, 8) == 3, "bf16 width sets");
static_assert(edge_chain_bf16_bwd_supported(640, 128, 448, 256, 64) && !edge_chain_bf16_bwd_supported(636, 128, 448, 256, 64) &&
              edge_chain_bf16_bwd_supported(316, 64, 224, 128, 32), "the 256-d form takes multiples of 32 only");
// image sizes in floats (fp32 | split) and chunk counts
static_assert(chain_floats(320 * 64, false) == 20480 && chain_floats(320 * 64, true) == 30720, "w2T at 128-d");
static_assert(chain_floats(96 * 32, false) == 3072 && chain_floats(96 * 32, true) == 4608, "w2T at 32-d");
static_assert(chain_f4(ChainFwd::KC1 * 320, false) == 1280 && chain_f4(ChainFwd::KC1 * 320, true) == 1920, "one phase-1 chunk at 128-d");
static_assert(chain_nchunks(320, ChainFwd::KC2) == 5 && chain_nchunks(160, ChainFwd::KC2) == 3 && chain_nchunks(96, ChainFwd::KC2) == 2, "phase-2 chunks");
static_assert(chain_wf1_blocks(224) == 4 && chain_wf1_block_cols(224, 3) == 32 && chain_wf1_blocks(128) == 2 && chain_wf1_blocks(64) == 1, "flow layer-0 block images");
static_assert(chain_wf1_block_off(64, 2, false) == 8192 && chain_wf1_block_off(64, 2, true) == 12288, "flow layer-0 block offsets at 128-d");
static_assert(chain_w1e_passes(128) == 2 && chain_w1e_cols(128) == 64 && chain_w1e_passes(64) == 1 && chain_w1e_passes(32) == 1 && chain_w1e_cols(32) == 32,
              "w1e pass images at 128-d / 64-d and 32-d (two halves) / one 32-wide half");
static_assert(chain_w1e_off(1, 320, 64, 64, false) == 24576 && chain_w1e_off(1, 320, 64, 64, true) == 36864, "w1e pass 1, row 64 at 128-d");
static_assert(chain_row_off(64, 320, true) == 30720, "Q0 row offset into w1T at 128-d");

}  // namespace mpnhip
