// gf_delta.hpp -- host-side interface of the delta-accumulate kernels (gf_delta.hip).
//
// The products behind EncodeIdx and Update (KRS/reedsolomon.go:631-667, 672-734): for every stripe s
//
//     delta:  d[c] = old[s][c] ^ new[s][c];  old[s][c] = d[c]      (c over the nc changed columns)
//     plain:  d[c] = in[s][c]
//     out[s][r][b] ^= XOR_c coef[r][c] * d[c][b]                   (r over the m output rows)
//
// in one pass: every byte of old, new and out is read once, every byte of old and out written once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cfsec {

struct DeltaJob {
  int nc = 0;                            // columns (inputs) per stripe
  int m = 0;                             // output rows per stripe, all accumulated into
  const uint8_t* coef = nullptr;         // host, m x nc row-major
  size_t len = 0;                        // bytes per row
  int nstripes = 0;
  uint8_t* const* old = nullptr;         // host array [nstripes * nc] of device pointers: delta: the old
                                         // columns, left holding old ^ new; plain: the inputs, read only
  const uint8_t* const* neu = nullptr;   // host array [nstripes * nc]: the new columns; NULL: a plain job
  uint8_t* const* out = nullptr;         // host array [nstripes * m]
  bool delta() const { return neu != nullptr; }
};

// Rows one launch carries: columns (dev::kMaxK) and accumulated rows (a lane's accumulators).
constexpr int kDeltaMaxCols = 32;
constexpr int kDeltaMaxRows = 32;
constexpr uint32_t kDeltaTile = 4096;  // bytes of every row per workgroup: 256 lanes x 16 bytes

// One launch: rows [r0, r0 + mc) x columns [c0, c0 + kc) of stripes [s0, s0 + ns), bytes [0, len).
// `delta`: the launch forms old ^ new of its columns and stores it back; else it reads them as they
// stand (a plain job, or a later row chunk of a delta job, whose columns an earlier launch rewrote).
struct DeltaStep {
  int r0, mc, c0, kc, s0, ns;
  bool delta;
  int M;             // accumulator rows of the kernel instantiation that runs the step (>= mc)
  int OS;            // waves of a workgroup sharing one column chunk: always 1 (the in-place hazard)
  uint64_t len;
  int64_t sstride;   // != 0: an affine run (one pointer set, any stripe count)
  uint32_t tile;     // bytes of every row per workgroup
  uint32_t grid_x, grid_y;  // tiles of a row, stripes
};
using DeltaVisitor = hipError_t (*)(const DeltaStep& step, void* ctx);  // != hipSuccess ends the plan

// The launches of a job, in order: a pure host function (no HIP calls; it reads the job's scalar
// fields and the pointer arrays' values).  Column chunks of kDeltaMaxCols outermost, each with its row
// chunks of kDeltaMaxRows (the first forms the chunk's deltas, the later ones are plain), each with
// its stripe runs: every stripe of an affine job at once (65535 per launch), else as many as the
// argument block's pointer slots hold at (2 kc + mc) pointers per stripe of a delta step, (kc + mc)
// of a plain one.  Returns the error launch_delta returns for the job, or the visitor's.
hipError_t plan_delta(const DeltaJob& job, DeltaVisitor visit, void* ctx);
// An instantiation with M accumulator rows exists (both modes).
bool delta_kernel_exists(int M);
// Enqueue the job on `stream`: fills one argument block per step and launches it.
// CFSEC_TRACE_DELTA (read per call) prints one stderr line per launch:
// "cfsec: delta mode=<delta|plain> nc=.. m=.. r0=.. c0=.. stripes=.. s0=.. len=.. affine=..".
hipError_t launch_delta(const DeltaJob& job, hipStream_t stream);

}  // namespace cfsec
