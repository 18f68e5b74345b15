// The kernel-selection switches of libdiagan_hip.so: every DIAGAN_* environment variable the host code reads for a selection query,
// defined once with its default.  INTEGRATION.md section 2 lists them in this order.
#pragma once
#include <atomic>
#include <stdlib.h>
#include <type_traits>

namespace diagan {

// first of "this call's option, the process-wide setter, the default" that is set (a level below 0 is unset)
static inline int first_set(int per_call, int process, int dflt) { return per_call >= 0 ? per_call : (process >= 0 ? process : dflt); }

// An environment variable with its default, read ONCE at first use (never at load time: tools and tests set variables after the
// import) and immutable from then on.  After that first use a look-up is a load and a compare -- it sits on the launch path.
template <class T>
struct EnvLatch {
  const char* name;
  T dflt;
  std::atomic<bool> read{false};
  std::atomic<T> val{};
  T env() {
    if (!read.load(std::memory_order_acquire)) {    // (two threads here at once store the same value)
      const char* s = getenv(name);
      T v = dflt;
      if (s) {
        if constexpr (std::is_same<T, double>::value) v = atof(s);
        else v = atoi(s);
      }
      val.store(v, std::memory_order_relaxed);
      read.store(true, std::memory_order_release);
    }
    return val.load(std::memory_order_relaxed);
  }
};
// integer switch: this call's option, else the process-wide setter, else the environment
struct Switch : EnvLatch<int> {
  int get(int per_call = -1, int process = -1) { return first_set(per_call, process, env()); }
};
using SwitchF = EnvLatch<double>;                    // environment only

// ---- Winograd routes (conv_gemm.hip, conv_wino*.hip, conv_wgrad.hip) ----------------------------------------------------------------
inline Switch kWino{{"DIAGAN_WINO", 1}};                         // 0: implicit GEMM only (A/B runs); also the Winograd weight gradient
inline Switch kWinoPool{{"DIAGAN_WINO_POOL", 1}};                // 0: no convolution + average-pool launches (tile_cfg 11 / 12)
// one 512-thread workgroup per CU: below ~3/4 of the chip the implicit GEMM's smaller tiles win (8x8 / 4x4 blocks at
// batch 64: 128 workgroups, 325 vs 317 us; their data-gradients 330 vs 168 us)
inline Switch kWinoMinWgs{{"DIAGAN_WINO_MIN_WGS", 192}};
inline Switch kWinoSplit{{"DIAGAN_WINO_SPLIT", 1}};              // 0: the automatic choice takes no channel-split Winograd launch
inline Switch kWinoWgrad{{"DIAGAN_WINO_WGRAD", 1}};              // 0: no Winograd F(3x3,2x2) weight gradient
// F(4x4,3x3).  DIAGAN_WINO4=0 is a HARD off: in pick_cfg_geom_impl, wino4_pool_ok and wino4_upin_ok it is read beside -- not under --
// diagan_conv_gemm_set_wino4 and the per-call wino4 option, so neither turns the kernel back on (unlike DIAGAN_WINO, DIAGAN_GEMM_X3,
// DIAGAN_GEMM_X3B and DIAGAN_SPLITK_FUSED, which the setter and the per-call field override).
inline Switch kWino4{{"DIAGAN_WINO4", 1}};
inline Switch kWino4MinCi{{"DIAGAN_WINO4_MIN_CI", 64}};
inline Switch kWino4X3{{"DIAGAN_WINO4_X3", 0}};                  // 1: its 36 frequency GEMMs on the bf16 pipe, operands split in three
inline Switch kWino4Pool{{"DIAGAN_WINO4_POOL", 1}};              // 0: the pooled launches stay on the F(2x2) pooled kernels
inline Switch kWino4PoolMinWgs{{"DIAGAN_WINO4_POOL_MIN_WGS", 192}};
inline Switch kWino4Upin{{"DIAGAN_WINO4_UPIN", 1}};              // 0: no F(4x4) launch on the up-sampled input (tile_cfg 15)
// ---- implicit GEMM (conv_gemm.hip, conv_gemm_x3*.hip) -------------------------------------------------------------------------------
inline Switch kSplit128{{"DIAGAN_SPLIT128", 0}};                 // on only for values > 0: split-K 128x128 tiles (opt-in, see pick_cfg)
inline Switch kKg2{{"DIAGAN_KG2", 1}};                           // 0: no two-K-group workgroups (tile_cfg 14)
inline Switch kKsplit{{"DIAGAN_KSPLIT", 0}};                     // tuning experiments only: forced split-K factor
inline Switch kSplitkFused{{"DIAGAN_SPLITK_FUSED", 0}};          // in-kernel split-K combine: off, it buys nothing (see splitk_tickets)
inline Switch kGemmX3{{"DIAGAN_GEMM_X3", 1}};                    // on: SNGAN-32 5270-5281 -> 5355 images/s
// (DIAGAN_GEMM_X3_RESIDENT, the form of the tile_cfg 16 kernel, selects no tile configuration and changes no selection query's answer:
//  it is defined in conv_gemm.hip beside its setter, outside the table the selection fixture tests/golden/conv_selection.json goes by)
inline Switch kGemmX3b{{"DIAGAN_GEMM_X3B", 1}};
inline Switch kGemmX3bMinTiles{{"DIAGAN_GEMM_X3B_MIN_TILES", 192}};
inline Switch kX3Pieces{{"DIAGAN_X3_PIECES", 3}};                // pieces per operand of the large split-operand kernels: 3, or 2 (opt-in)
inline Switch kGemmX3bForm{{"DIAGAN_GEMM_X3B_FORM", 0}};         // 1 / 2 force a form of the tile_cfg 17 kernel, 0: automatic
inline Switch kGemmX3bForm2Tiles{{"DIAGAN_GEMM_X3B_FORM2_TILES", 512}};
inline Switch kConvCi4{{"DIAGAN_CONV_CI4", 1}};                  // 0: no direct 3x3 kernel for 4 input channels (conv_small.hip)
// ---- weight gradient (conv_wgrad.hip, conv_wgrad_x3.hip) ----------------------------------------------------------------------------
inline Switch kWgradMinSteps{{"DIAGAN_WGRAD_MINSTEPS", 4}};      // at least this many K-steps per split
inline SwitchF kWgradFixed{"DIAGAN_WGRAD_FIXED", 6.0};           // fixed cost of a block in K-steps (diagan_conv_wgrad_splits)
inline Switch kWgradX3{{"DIAGAN_WGRAD_X3", 1}};
inline SwitchF kWgradX3MinMac{"DIAGAN_WGRAD_X3_MIN_MAC", 4e9};   // below: the launch, not the matrix pipe, is what the time goes to
// ---- other kernels ------------------------------------------------------------------------------------------------------------------
inline Switch kFirRows{{"DIAGAN_FIR_ROWS", 1}};                  // 0: one output row per lane in the blur kernels (A/B; default: four)
// a thread walks rows_per_split / (256 / columns) rows, four loads in flight: with 256 rows per split and 1024 blocks a
// 65536 x 256 reduction was 16 dependent iterations = 21 us; 128 / 2048: SNGAN-32 +0.8 %, SNGAN-64 +0.2 % end to end
// (64 / 4096: +1.0 % / -0.45 %; tools/probe/colred_sweep.sh)
inline Switch kColredBlocks{{"DIAGAN_COLRED_BLOCKS", 2048}};
inline Switch kColredRows{{"DIAGAN_COLRED_ROWS", 128}};

}  // namespace diagan
