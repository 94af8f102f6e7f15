// fft_path.hpp — what the FFT path's unit (fft_path.hip: the kernels and their launchers) and the handle's unit (vqt_engine.hip:
// batch_streams_device builds the stream table) share.  Included by those two only; nothing here is a kernel.
#pragma once

#include "device_tables.hpp"

namespace pvq {

// many streams in one launch of the FFT path: frames are numbered through all streams; stream i holds the frames from frame0
struct FftStream {
    const float* pcm;
    long long n_lead, n_samples;
    long long row0;     // output row of its frame 0
    long long frame0;   // global index of its frame 0 (ascending over the table)
};
struct FftArgs {
    const FftStream* streams;   // nullptr: one stream, described by the fields below
    int n_streams;
    const float* pcm;
    long long n_lead;
    long long hop;
    long long n_samples;  // total samples in pcm (for upper-bound safety)
    int n_fft;
    int n_frames;
    int n_groups;
    int n_bins;
    int n_tw;       // twiddle table length (= largest complex FFT size)
    int max_cols;   // LDS spec capacity
    const GroupDev* groups;
    const float2* tw;
    const float2* split_tw;
    const uint32_t* row_ptr;
    const float4* ent;   // (re, im, column | conj flag, -) per kernel entry
    float* out_db;
    float2* out_cplx;
    unsigned* status;
    int dev_skip;   // developer knob PVQ_FFT_SKIP (timing experiments, wrong results): 1 skips the row dots, 2 the FFT passes
    // Few frames (the streaming front end's single frame, short clips): one workgroup per (frames of a workgroup, WINDOW GROUP) instead
    // of one walking the groups in turn — a frame's latency is then its longest group's (the 16 384-sample window: ~55 % of the
    // walk), not their sum; x_vqt goes through xv_split ([frame][bin], complex) and db_rows finishes the frames.  Same arithmetic
    // per group, same dB routine: same bits as the walk.
    float2* xv_split;   // nullptr: every workgroup walks all groups
};

}  // namespace pvq
