// dnn_host.h -- the host side of DNN scoring: the object, which dnn_api.hip builds and owns (validation, the packed
// weights, scratch, the side stream of a long batch, the C ABI of jamd_dnn), and the launchers through which it reaches
// the kernels in dnn.hip.  The API unit launches nothing itself; a launcher checks nothing.  Internal, not installed.
#pragma once
#include "jamd_host.h"

constexpr int kDnnRowBlock = 128;          // frames (and outputs) of a block tile: a chunk of a long batch is a multiple
constexpr int kDnnSlab = 32;               // entries of one residue segment per slab

// Place of entry m inside its residue segment (dnn.hip, "residue-major" rows): inside each group of eight the even
// ones come first.  One definition for the host's weight packing and the hidden layers' epilogue.
__host__ __device__ __forceinline__ int dnn_rm_pos(int m) {
  const int e = m & 7;
  return (m & ~7) | ((e & 1) ? 4 + (e >> 1) : (e >> 1));
}

struct JAMD_LOCAL jamd_dnn {
  jamd_engine *eng = nullptr;
  int nlayer = 0;
  std::vector<int> dims;
  std::vector<JamdDev<float>> d_b;
  std::vector<JamdDev<float>> d_wr;  // W[l] in residue-major rows (see dnn_layer_rs_kernel), [dims[l+1]][8 * kmp[l]]
  std::vector<int> kmp;            // per layer input: padded length of one residue segment = ceil(dims[l] / 8 / 8) * 8
  JamdDev<float> d_xr;             // the frames in residue-major rows
  JamdDev<float> d_prior;
  JamdDev<float> d_zero;           // 64 zero bytes: DMA source of out-of-range quads
  int maxdim = 0;
  JamdDev<float> d_act[2];         // hidden activations ping-pong between two [T][maxhidden] buffers
  JamdDev<float> d_lse;
  JamdStage<float, float> stage;   // outprob_host
  hipStream_t side = nullptr;          // softmax tail of chunk c runs here while chunk c+1's GEMMs run on the caller's stream
  hipEvent_t ev_gemm[8] = {}, ev_tail = nullptr, ev_start = nullptr;
};

// ---- dnn.hip
// Frames t0 ... t0 + Tc of dev_frames: packed into n->d_xr, then every layer; the output layer's raw values -> dev_out
JAMD_LOCAL int dnn_launch_layers(jamd_dnn *n, hipStream_t st, const float *dev_frames, int t0, int Tc, float *dev_out);
// The row log-sum (n->d_lse) and the normalisation of the same rows of dev_out
JAMD_LOCAL int dnn_launch_tail(jamd_dnn *n, hipStream_t ts, int t0, int Tc, float *dev_out);
