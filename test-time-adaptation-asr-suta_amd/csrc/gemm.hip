// GEMM dispatcher.  gemm_route() decides once which kernel a GEMM takes -- family, tile, stage variant, split-K,
// tile order, grid (GemmRoute, common.h) -- and gemm_launch() launches what the route says.
//   operands                               family              chosen by
//   MN-contiguous bf16 planes (ta, !tb)    hbt4 | hbt          hbt4_ok and a full round of 256^2 tiles (SUTA_HBT4)
//   k-contiguous bf16 planes, conv-A rows  hbx | hb            hbx_conv_wins (SUTA_HBX, SUTA_HBP_CONV)
//   k-contiguous bf16 planes               hbx | hb            hbx_wins (SUTA_HBX, SUTA_HBX_T); hb's tile: HB_TILES
//   fp32, mode 2 (bf16 products)           gbf | x6_1plane     gbf: transposed A, LDS-DMA-able; tile: BF16_TILES
//   fp32, mode 1 (x6)                      x6                  tile: X6_TILES
//   fp32, mode 0 (exact)                   f32p | glds | f32   f32p_wins (SUTA_F32P); glds: LDS-DMA-able; GLDS_TILES
// The eligibility rules of the 256 x 256 kernels (hbx, hbx16, hbt4, f32p) are gemm_hbx.hip's *_ok predicates; which
// instantiation of them a route is comes from hbx_resolve there.  Forced variants (gemm_set_variant: tools/gemm_bench,
// tools/hb_bench) are translated there into a tile, a 256 x 256 request and a stage number, and enter gemm_route in two
// places: the tile replaces the tile choice of the last four rows (a forced run takes no hbt4, CONV form or f32p), and
// stage_override() picks each family's stage variant (the number also selects the benchmark families gbf / gbf_x6).
#include "gemm_kernels.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

namespace {

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

struct TileCand {
    int bm, bn;
    double eff;  // relative MFMA efficiency of the tile
};

// gemm_set_variant(tile, nbuf): whether a tile is forced, the tile, and the MFMA rows (32 / 16) of a forced request for
// the 256 x 256 bf16-plane kernel (0: none)
bool g_forced = false;
TileCand g_tile = {128, 128, 0.0};
int g_tile256 = 0;
int g_nbuf = 3;  // 3 = LDS-DMA kernel where its preconditions hold (else the register-staged one)
int g_mode = 0;  // 0 = exact fp32 MFMA, 1 = x6 (fp32-accurate bf16 split), 2 = bf16 products

}  // namespace

void gemm_set_variant(int tile, int nbuf) {
    // the benchmarks' tile numbers, translated here and nowhere else: {BM, BN, MFMA rows of a 256 x 256 request} by
    // number (6 and 7 name no tile).  8 / 9 ask for the 256 x 256 bf16-plane kernel on 32x32x16 / 16x16x32 MFMAs; on a
    // GEMM that kernel cannot run (gemm_route: hbx_can_run) the request falls back to the 128 x 128 they carry here.
    static const int ids[10][3] = {{128, 128, 0}, {128, 64, 0}, {64, 128, 0}, {64, 64, 0},     {256, 128, 0},
                                   {128, 256, 0}, {0, 0, 0},    {0, 0, 0},    {128, 128, 32}, {128, 128, 16}};
    if (tile > 9 || (tile >= 0 && !ids[tile][0])) throw std::invalid_argument("gemm_set_variant: no such tile");
    g_forced = tile >= 0;
    g_tile = g_forced ? TileCand{ids[tile][0], ids[tile][1], 0.0} : TileCand{128, 128, 0.0};
    g_tile256 = g_forced ? ids[tile][2] : 0;
    g_nbuf = nbuf;
}

// Kernel census (suta_set_census / suta_get_census): host-side count of GEMM launches per
// (kernel, tile, batch count, split count, operand form), so a test can assert which instantiation a
// layout reaches.  Counted when a launch is issued (eager or while a graph is captured), not on replay.
static std::mutex g_census_mu;
static std::map<std::string, long> g_census;
static std::atomic<bool> g_census_on{false};
// with engine timing on as well: per GEMM shape, the summed HIP-event time of its launches ("ms|<shape>|n=<n>"
// entries, value in microseconds)
static std::map<std::string, std::pair<double, long>> g_census_ms;

void gemm_census_enable(bool on) {
    std::lock_guard<std::mutex> lk(g_census_mu);
    g_census_on = on;
    g_census.clear();
    g_census_ms.clear();
}

bool gemm_census_is_on() { return g_census_on; }

void gemm_census_time(const std::string& shape, double ms) {
    std::lock_guard<std::mutex> lk(g_census_mu);
    auto& e = g_census_ms[shape];
    e.first += ms;
    e.second += 1;
}

std::string gemm_census_text() {
    std::lock_guard<std::mutex> lk(g_census_mu);
    std::string out;
    for (const auto& kv : g_census) out += kv.first + " " + std::to_string(kv.second) + "\n";
    for (const auto& kv : g_census_ms)
        out += "ms|" + kv.first + "|n=" + std::to_string(kv.second.second) + " " +
               std::to_string((long)(kv.second.first * 1000.0)) + "\n";
    return out;
}

const char* gemm_family_name(GemmFamily f) {
    static const char* const names[] = {"f32", "glds", "x6", "x6_1plane", "gbf", "gbf_x6", "hb", "hbt", "hbt4", "hbx",
                                        "hbx16", "f32p"};
    return names[f];
}

// Each launch also counts one "grid <kernel> <BMxBN> gx=<column tiles> gy=<row tiles> z=<Z> split=<k>" entry, so
// a test can assert the tile grid a layout reaches (e.g. the 512 row tiles of 164 x 399 frames).
// and one "epi <kernel> <BMxBN> <epilogue flags>" entry (e.g. EPI_DELTA = 256 on hbx: the fused flash-backward delta ran).
static void census(const GemmRoute& r, const GemmParams& p) {
    if (!g_census_on) return;
    const char* kernel = gemm_family_name(r.family);
    char key[160], gkey[160], ekey[96];
    snprintf(key, sizeof key, "%s %dx%d z=%ld split=%d %s%s%s", kernel, r.BM, r.BN, (long)p.Z, r.splits,
             p.ta ? "T" : "N", p.tb ? "T" : "N", p.segK > 0 ? (p.segB ? " conv-seg" : " conv") : "");
    snprintf(gkey, sizeof gkey, "grid %s %dx%d gx=%u gy=%u z=%ld split=%d", kernel, r.BM, r.BN, r.gx, r.gy, (long)p.Z,
             r.splits);
    snprintf(ekey, sizeof ekey, "epi %s %dx%d %d", kernel, r.BM, r.BN, p.epi);
    std::lock_guard<std::mutex> lk(g_census_mu);
    ++g_census[key];
    ++g_census[gkey];
    ++g_census[ekey];
}

void gemm_set_mode(int mode) { g_mode = mode; }
int gemm_get_mode() { return g_mode; }

void gemm_init(GemmParams& p) {
    p = GemmParams{};
    p.Z = 1;
    p.zdiv = 1;
    p.alpha = 1.f;
    p.splits = 1;
    p.mode = g_mode;
}

// ---- tile choice ----
// time ~ blocks charged x tile area / eff.  whole_rounds: a grid is charged whole rounds of `round` resident blocks;
// else it is charged its tiles, and one full round where it has fewer.
static long tiles_of(const GemmParams& p, int bm, int bn) {
    return (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) * p.Z;
}
static double tile_cost(const TileCand& c, const GemmParams& p, long round, bool whole_rounds) {
    const long tiles = tiles_of(p, c.bm, c.bn);
    const long charged = whole_rounds ? (tiles + round - 1) / round * round : std::max(tiles, round);
    return (double)charged * c.bm * c.bn / c.eff;
}
// the first candidate (rows up to max_bm) no later one beats by more than 0.1 %
template <int N>
static TileCand best_tile(const TileCand (&cands)[N], const GemmParams& p, long round, bool whole_rounds,
                          int max_bm = 256) {
    int best = 0;
    double bt = 1e300;
    for (int i = 0; i < N; ++i) {
        if (cands[i].bm > max_bm) continue;
        const double t = tile_cost(cands[i], p, round, whole_rounds);
        if (t < bt * 0.999) {
            bt = t;
            best = i;
        }
    }
    return cands[best];
}
// the grid fills one round of 256 tiles of 256^2: where the 256 x 256 kernels (one block per CU) are chosen unforced
static bool fills_256_round(const GemmParams& p) { return tiles_of(p, 256, 256) >= 256; }

// eff measured with tools/gemm_bench on the SUTA shapes at 64 utterances: 128x128 wins every large GEMM despite its
// coarser tail; smaller tiles win where M or N is below ~128, e.g. attention and the 48-channel positional-conv
// groups.  Charged per tile, a grid with fewer tiles than the 256 CUs as one full round of them.
static const TileCand GLDS_TILES[4] = {{128, 128, 1.0}, {128, 64, 0.93}, {64, 128, 0.92}, {64, 64, 0.85}};
static const TileCand X6_TILES[4] = {{128, 128, 1.0}, {128, 64, 0.9}, {64, 128, 0.9}, {64, 64, 0.75}};
// bf16 mode (tools/gemm_bench, 64 utterances): the register-staged one-plane kernel beats the LDS-DMA
// fp32-staged one on every operand layout except transposed A (weight gradients, TN), and its
// 256x128 tile (wave tile 128x64: 1.3x fewer L2 bytes per flop) wins wherever the grid still fills
// whole rounds of 512 resident blocks (2 per CU): 420-430 TF on FFN1 / QKV / conv1 vs 360-390.
// Charged in whole rounds of 512 blocks.
static const TileCand BF16_TILES[5] = {{128, 128, 1.0}, {256, 128, 1.12}, {128, 64, 0.85}, {64, 128, 0.85}, {64, 64, 0.6}};
// bf16-plane GEMMs (tools/hb_bench, C4 linears at M = 25536): 128x128 with two LDS stages wins every
// shape (460-660 TF vs 370-570 for 256x128 at one block per CU); smaller tiles only for small grids.
static const TileCand HB_TILES[4] = {{128, 128, 1.0}, {128, 64, 0.85}, {64, 128, 0.85}, {64, 64, 0.6}};

// ---- which GEMMs take a 256 x 256 kernel (the operand conditions are gemm_hbx.hip's) ----

// A bf16-plane linear the 256 x 256 kernels can run: plain rows, K in whole 32-deep slices and at least four of them;
// batched (Z > 1) GEMMs -- the conv stack's per-utterance forward -- only on the four-phase form with the staged C^T
// epilogue (32x32x16 MFMAs only).  Asked of unforced and forced requests alike.
static bool hbx_can_run(const GemmParams& p, int mfma_rows) {
    return p.segK == 0 && p.K % 32 == 0 && p.K >= 128 && (p.Z == 1 || (mfma_rows == 32 && hbx_four_phase_ok(p)));
}

// 256 x 256 slice-ring bf16-plane kernel (gemm_hbx.hip, v_mfma_f32_32x32x16_bf16; bitwise the 128 x 128 kernel's
// results: same MFMA products, same k order) for the linears on grids of at least one full round of 256 tiles.
// tools/hb_bench (C4 shapes at M = 164 x 399, same box; profiles/r4/hbx_epilogue_hb_bench.log): qkv 729 -> 875 TF,
// out-proj 597 -> 770, FFN1 759 -> 854, FFN2 866 -> 1065, dQKV 819 -> 1003.  The GELU / GELU' linears need its C^T
// epilogue with LDS-staged whole-line stores (SUTA_HBX_T=2): FFN1 (bias + GELU + bf16 pre) 603 -> 737 TF, FFN2 input
// gradient 611 -> 719; the column-per-lane epilogue (two-lane-pair dword stores, 2 rows per instruction) measured
// 595 / 627 and direct row-per-lane 16-B stores (32 rows per instruction) 515 / 625, so without the staged form
// they keep the 128 x 128 kernel.
// SUTA_HBX=0: off (A/B runs); 2: every eligible linear, any epilogue and grid (tests).
static bool hbx_wins(const GemmParams& p) {
    const SutaSwitches& sw = suta_switches();
    if (!sw.hbx || !hbx_can_run(p, 32) || (p.epi & (EPI_ACCUM | EPI_SMBWD))) return false;
    if (sw.hbx == 2) return true;
    if ((p.epi & (EPI_GELU | EPI_DGELU | EPI_STORE_PRE)) && !(sw.hbx_t == 2 && hbx_t_ok(p))) return false;
    return fills_256_round(p);
}

// the conv stack's input gradients (conv-A rows, per-tap weight segments: config C4's conv-seg GEMMs, Z = B) on the
// four-phase 256 x 256 kernel's CONV form (hbp_conv_ok) on grids of at least one round of 256 tiles;
// SUTA_HBP_CONV=0 keeps them on the 128 x 128 kernel (A/B runs), SUTA_HBX=2 forces them on every eligible grid
static bool hbx_conv_wins(const GemmParams& p) {
    const SutaSwitches& sw = suta_switches();
    return sw.hbx && sw.hbp_conv && hbp_conv_ok(p) && (sw.hbx == 2 || fills_256_round(p));
}

// The exact-fp32 GEMMs on the four-phase 256 x 256 kernel's fp32 forms (f32p_form: bitwise the 128 x 128
// LDS-DMA kernel's results -- the same v_mfma_f32_32x32x2_f32 products in the same k order) on grids of at least one
// round of 256 tiles: one block per CU whose two wave groups run a barrier apart, so one group's fragment reads and DMA
// issue sit under the other's MFMAs, and whole-line staged stores, against two co-resident 128 x 128 blocks whose
// prologues and epilogues coincide.
// SUTA_F32P=0: off (A/B runs); 2: every eligible GEMM on any grid (tests).
// Forward (NT) linears with K < 1024 -- wav2vec2-base's QKV, out-projection and FFN1 -- stay on the 128 x 128 kernel:
// tests/test_gpu_bench_scale.py::test_bench_layout_matches_oracle asserts the bench layout's census still holds
// "grid glds 128x128" entries with gx = 6, 18 and 24 at gy = 512 (QKV forward is the only gx = 18 GEMM); a change
// that may touch that test lifts this rule.
static bool f32p_wins(const GemmParams& p) {
    const int mode = suta_switches().f32p;
    if (!mode || g_forced || g_nbuf != 3 || !f32p_form(p)) return false;
    if (mode == 2) return true;
    if ((p.tb && p.segK == 0 && p.K < 1024) || !fills_256_round(p)) return false;
    // A 256-row tile pads short conv layers more than the 128- and 64-row tiles do (799 rows: 1024 against 896), so
    // the kernel is kept where its padded area over its relative rate beats the best 128 x 128-family tile's.
    // Rates from the eager trace of the bench layout (profiles/r7, ms per launch against the
    // 128 x 128 kernel at equal padded area): conv-seg input gradients -8 to -10 %, linears and the conv forward -2 to
    // -4.5 %; at 3199 / 1599 / 799 / 399 rows the conv forward measured +1 / +1 / +23 / +36 % and stays where it was.
    const double eff = p.segK > 0 ? 1.05 : 1.03;
    double best = 1e300;
    for (const TileCand& c : GLDS_TILES) best = std::min(best, tile_cost(c, p, 256, false));
    return (double)tiles_of(p, 256, 256) * 65536.0 / eff < best;
}

// 32-bit epilogue offsets: M x ld elements of every operand the epilogue touches within 4 GiB
// (SUTA_EPI_FAST=0 in the call's switch snapshot: the general epilogue everywhere, for A/B runs)
static int epilogue_off32(const GemmParams& p) {
    const int fast = suta_switches().epi_fast;
    const double lim = 4294967295.0 - 1024.0;
    auto fits = [&](long ld, double esz) { return (double)p.M * (double)std::max(ld, (long)p.N) * esz < lim; };
    return fits(p.ldc, 4) && (!(p.epi & EPI_RESID) || fits(p.ldr, 4)) &&
           (!(p.epi & (EPI_DGELU | EPI_SMBWD)) || fits(p.ldaux, 4)) && (!(p.epi & EPI_STORE_PRE) || fits(p.ldc2, 4)) &&
           (!(p.epi & EPI_DELTA) || fits(p.ldo, 4)) && (!p.Cb || fits(p.ldcb, 2)) && p.ldc >= 0 && p.ldr >= 0 &&
           p.ldaux >= 0 && p.ldc2 >= 0 && p.ldcb >= 0 && p.ldo >= 0 && fast;
}

// ---- stage variants: the defaults, and gemm_set_variant's nbuf where a benchmark sets one ----
static void stage_override(GemmRoute& r) {
    const int nb = g_nbuf;
    r.stages = 2, r.bk = 32;
    switch (r.family) {
    case GF_HB: {
        // SUTA_HB_NS: stage variant of the 128 x 128 bf16-plane kernel (A/B runs; 2 default), read once (thread-safe)
        static const int hbns = [] {
            const char* ev = std::getenv("SUTA_HB_NS");
            return ev ? std::max(2, atoi(ev)) : 2;
        }();
        // 3 = three stages, 4 = 64-deep K-steps, 5 / 6 = 16-deep K-steps on 4 / 3 stages (128 x 128 only)
        const int ns = g_forced ? nb : (r.BM == 128 && r.BN == 128) ? hbns : 2;
        if (r.BM + r.BN > 256) break;  // 256 x 128, 128 x 256: two 32-deep stages only
        if (ns == 3) r.stages = 3;
        if (ns == 4) r.bk = 64;
        if (ns == 5 || ns == 6) r.stages = ns == 5 ? 4 : 3, r.bk = 16, r.BM = r.BN = 128;
        break;
    }
    case GF_X6_1PLANE: r.stages = 1; break;
    case GF_GBF: r.bk = nb == 8 ? 64 : 32; break;       // benchmark variant 8 = BK64 x 2
    case GF_GBF_X6: r.bk = nb == 10 ? 64 : 32; break;   // benchmark variants 9 = BK32 x 2, 10 = BK64 x 2
    case GF_X6: r.stages = nb == 2 ? 2 : 1, r.bk = nb == 2 ? 16 : 32; break;  // BK 16 double-buffered | BK 32, one stage
    case GF_GLDS:  // 3 = BK32 x 2 stages, 4 = BK16 x 4, 5 = BK16 x 3, 6 = BK32 x 3, 7 = BK64 x 2
        r.stages = nb == 4 ? 4 : (nb == 5 || nb == 6) ? 3 : 2;
        r.bk = (nb == 4 || nb == 5) ? 16 : nb == 7 ? 64 : 32;
        break;
    case GF_F32: r.stages = nb == 2 ? 2 : 1; break;
    default: break;
    }
}

GemmRoute gemm_route(const GemmParams& p0, bool have_ws, long ws_floats) {
    GemmParams p = p0;
    const SutaSwitches& sw = suta_switches();
    const int second = ((p.epi & EPI_RESID) != 0) + ((p.epi & EPI_ACCUM) != 0) + ((p.epi & EPI_SMBWD) != 0);
    if (second > 1 || ((p.epi & EPI_SMBWD) && p.epi != EPI_SMBWD))
        throw std::invalid_argument("gemm epilogue: RESID / ACCUM / SMBWD are mutually exclusive");
    auto vec_ok = [](const float* base, long ld, long s0, long s1) {
        return aligned16(base) && (ld % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0);
    };
    p.va = vec_ok(p.A, p.lda, p.sA0, p.sA1) && (p.segK == 0 || p.segK % 4 == 0);
    p.vb = vec_ok(p.B, p.ldb, p.sB0, p.sB1) && (!p.segB || (p.sBseg % 4 == 0 && p.segK % 4 == 0));

    const bool glds_ok = p.va && p.vb && (p.ta || p.K % 4 == 0) && (!p.tb || p.K % 4 == 0);
    const bool hbt = p.mode == 2 && p.Ab && p.Bb && p.ta && !p.tb;  // MN-contiguous bf16 planes (gemm_hbt_kernel)
    const bool hb = p.mode == 2 && p.Ab && p.Bb && !p.ta;            // k-contiguous bf16 planes (gemm_hb_kernel)
    if (p.mode == 2 && p.Ab && p.Bb && !hb && !hbt)
        throw std::invalid_argument("gemm: bf16 planes: A and B both k-contiguous ([M][K], [N][K]) or both MN-contiguous");
    if (hbt && (p.M % 8 || p.N % 8 || p.ldab % 8 || p.ldbb % 8 || !aligned16(p.Ab) || !aligned16(p.Bb) || p.Cb ||
                ((p.sA0 | p.sA1 | p.sB0 | p.sB1) % 8)))
        throw std::invalid_argument("gemm: MN-contiguous bf16 planes need M, N, ld, batch strides % 8 == 0, 16-B alignment");
    if (p.Cb && (!hb || (p.Z != 1 && (p.sCb1 % 4 || p.zdiv != 1)) || (reinterpret_cast<uintptr_t>(p.Cb) & 7)))
        throw std::invalid_argument("gemm: a bf16 output plane needs the bf16-plane kernel, 8-B alignment (Z > 1: sCb1 % 4 == 0)");
    if (hb && (p.K % 8 || p.ldab % 8 || p.ldbb % 8 || !aligned16(p.Ab) || !aligned16(p.Bb) ||
               (p.Z > 1 && ((p.sA0 | p.sA1 | p.sB0 | p.sB1) % 8))))
        throw std::invalid_argument("gemm: bf16 planes need K, ld and batch strides % 8 == 0 and 16-B alignment");
    p.off32 = epilogue_off32(p);  // before the kernel choice: the 256 x 256 kernels' rules ask it
    p.fgelu = sw.fast_gelu;       // (the engine call's switch snapshot)
    if (p.preb && (!hb || !p.Cb || (p.ldc2 & 1)))
        throw std::invalid_argument("gemm: bf16 pre-activation operands need the bf16-plane kernel with a Cb plane, ldc2 even");
    if (hb && p.segK > 0 && (p.segK % 8 || p.pad < 0 || (p.segB && (p.sBseg % 8))))
        throw std::invalid_argument("gemm: conv-A bf16 planes need segK and the tap stride % 8 == 0");

    // the family and its tile.  The first three rows never take a forced tile; the others take forced_tile where one
    // is set, except that a forced 256 x 256 request the kernels cannot run falls back to 128 x 128 (g_tile) -- the
    // unforced choices ask the same hbx_can_run.
    GemmRoute r{};
    TileCand t = {128, 128, 1.0};
    const bool x256 = g_tile256 && hb && hbx_can_run(p, g_tile256);  // a forced 256 x 256 request that can run
    if (f32p_wins(p)) {
        r.family = GF_F32P;
    } else if (hbt) {
        // conv weight gradients: the four-phase 256 x 256 TN form on grids that fill the chip (a smaller grid keeps
        // the 128 x 128 kernel with its split-K); SUTA_HBT4=2: on every grid (tests)
        r.family = (!g_forced && hbt4_ok(p) && (sw.hbt4 == 2 || fills_256_round(p))) ? GF_HBT4 : GF_HBT;
    } else if (hb && p.segK > 0) {
        r.family = (!g_forced && hbx_conv_wins(p)) ? GF_HBX : GF_HB;
    } else if (hb) {
        r.family = x256 ? (g_tile256 == 16 ? GF_HBX16 : GF_HBX) : (!g_forced && hbx_wins(p)) ? GF_HBX : GF_HB;
        t = g_forced ? g_tile : best_tile(HB_TILES, p, 512, true);
    } else if (p.mode == 2) {
        // bf16 products from fp32 operands: the register-staged one-plane kernel; weight gradients (transposed A)
        // on register-converted LDS-DMA stages, which have no 256 x 128 tile (benchmark variants 3 / 8 force them)
        const bool bf16_gbf = glds_ok && p.ta;
        t = g_forced ? g_tile : best_tile(BF16_TILES, p, 512, true, bf16_gbf ? 128 : 256);
        const bool gbf = glds_ok && t.bm + t.bn <= 256 && (g_forced ? (g_nbuf == 3 || g_nbuf == 8) : bf16_gbf);
        r.family = gbf ? GF_GBF : GF_X6_1PLANE;
    } else {
        // fp32-accurate: x6 (register splits on LDS-DMA stages: benchmark variants 9 / 10) or exact fp32 on the
        // LDS-DMA kernel where its loader's alignment holds
        r.family = p.mode == 1 ? ((glds_ok && g_nbuf >= 9) ? GF_GBF_X6 : GF_X6)
                               : ((glds_ok && g_nbuf >= 3) ? GF_GLDS : GF_F32);
        t = g_forced ? g_tile : best_tile(p.mode == 1 ? X6_TILES : GLDS_TILES, p, 256, false);
    }
    const bool is256 = r.family == GF_F32P || r.family == GF_HBT4 || r.family == GF_HBX || r.family == GF_HBX16;
    // (256 x 128 and 128 x 256 exist in the hb and x6_1plane families only; forced elsewhere: 128 x 128)
    if (t.bm + t.bn > 256 && r.family != GF_HB && r.family != GF_X6_1PLANE) t = {128, 128, 1.0};
    r.BM = is256 ? 256 : t.bm;
    r.BN = is256 ? 256 : t.bn;
    if (is256) hbx_resolve(r, p);
    else stage_override(r);
    if (r.family == GF_HB && p.segK > 0) r.stages = 2, r.bk = 32;  // (conv-A rows: the one instantiation)

    r.gx = (p.N + r.BN - 1) / r.BN;
    r.gy = (p.M + r.BM - 1) / r.BM;
    const long blocks = (long)r.gx * r.gy * p.Z;
    // split-K when the grid cannot fill 256 CUs and K is long
    // (the 256 x 256 kernels do not split; the split-K reduce has no bf16 pre store and no batched bf16 C plane)
    int splits = 1;
    if (have_ws && sw.splitk && p.K >= 1024 && blocks < 256 && !is256 && !p.preb && !(p.Cb && p.Z > 1)) {
        splits = (int)std::min<long>(16, (512 + blocks - 1) / blocks);
        while (splits > 1 && (long)splits * p.Z * p.M * (long)p.N > ws_floats) --splits;
        splits = std::min(splits, std::max(1, (p.K + 255) / 256));  // >= 256 K per split
    }
    r.kchunk = splits > 1 ? (((p.K + splits - 1) / splits + BK - 1) / BK) * BK : p.K;
    if (splits > 1) splits = (p.K + r.kchunk - 1) / r.kchunk;
    r.splits = splits;
    // tile order (xcd_tile): n-fastest by default (m-fastest and other band widths measured 1-4 % slower on the
    // fp32 linears).  bf16-plane GEMMs: bands of 8 tile rows (N >= 2048) or 4 walked column by column keep both operand
    // panels L2-resident (tools/hb_bench, M = 25 536: qkv 543 -> 598 TF, ffn1 525 -> 590, the N = 1024
    // shapes within +-2 %); the fp32 kernels measured neutral and keep the n-fastest order
    r.order = 0;
    if (hb && splits == 1) r.order = r.gx >= 16 ? 8 : 4;
    // fp32 linears with >= 16 column tiles (QKV, FFN1 and their input-gradient GEMMs): their weight panels do
    // not stay in an XCD's 4 MB L2 across a band of rows in n-fastest order; bands of 8 tile rows walked
    // column by column halve their HBM reads (FFN1 forward 1.43 -> 0.72 GB per launch, PMC) at equal time
    // (37.05 vs 37.13 utt/s, within noise); narrow GEMMs (6 column tiles) keep the n-fastest order, which
    // reads less for them
    if (!hb && p.mode == 0 && splits == 1 && p.Z == 1 && r.gx >= 16) r.order = 8;
    r.gz = p.Z * splits;
    r.off32 = p.off32;
    r.fgelu = p.fgelu;
    r.va = p.va;
    r.vb = p.vb;
    return r;
}

bool gemm_hbx_t_selected(const GemmParams& p) { return gemm_route_hbx_t(gemm_route(p, false, 0)); }

void gemm_launch(GemmParams p, hipStream_t st, float* ws, long ws_floats) {
    if (p.M <= 0 || p.N <= 0 || p.Z <= 0) return;
    const GemmRoute r = gemm_route(p, ws != nullptr, ws_floats);
    if ((p.epi & EPI_DELTA) && !gemm_route_hbx_t(r))
        throw std::invalid_argument("gemm: EPI_DELTA needs the 256 x 256 bf16-plane kernel's C^T epilogue (gemm_hbx_t_selected)");
    p.va = r.va, p.vb = r.vb, p.off32 = r.off32, p.fgelu = r.fgelu;
    p.splits = r.splits, p.kchunk = r.kchunk, p.order = r.order, p.ws = ws;
    census(r, p);
    const dim3 grid(r.gx, r.gy, r.gz);
    switch (r.family) {
    case GF_F32: gemm_run_f32(r.BM, r.BN, r.stages, p, grid, st); break;
    case GF_GLDS: gemm_run_glds(r.BM, r.BN, r.bk, r.stages, p, grid, st); break;
    case GF_X6: gemm_run_x6(r.BM, r.BN, r.bk, 3, p, grid, st); break;
    case GF_X6_1PLANE: gemm_run_x6(r.BM, r.BN, r.bk, 1, p, grid, st); break;
    case GF_GBF: gemm_run_gbf(r.BM, r.BN, r.bk, 1, p, grid, st); break;
    case GF_GBF_X6: gemm_run_gbf(r.BM, r.BN, r.bk, 6, p, grid, st); break;
    case GF_HB: gemm_run_hb(r.BM, r.BN, r.stages, r.bk, p, grid, st); break;
    case GF_HBT: gemm_run_hbt(p, grid, st); break;
    case GF_HBT4: case GF_HBX: case GF_HBX16: case GF_F32P: gemm_run_256(r, p, grid, st); break;
    }
    if (r.splits > 1) {
        const long MN = (long)p.M * p.N;
        const int gxr = (int)std::min<long>(1024, (MN + 255) / 256);
        hipLaunchKernelGGL(gemm_splitk_reduce, dim3(gxr, p.Z), dim3(256), 0, st, p);
    }
}
