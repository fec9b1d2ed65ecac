// fg_streams.hpp -- the scalar rules of a decode chunk that holds frames of several streams,
// shared by the device kernels (fg_dec_streams.hip), the host layer (fg_dec_host.cpp) and the
// stand-alone host program of the tests (tests/cpp/streams_host_main.cpp).  Compiles under hipcc
// and plain g++.
//
// All frames of all streams, in stream order, are cut into chunks of at most max_frames frames.
// The run of one stream's frames inside one chunk is a SEGMENT; a stream has at most one segment
// per chunk, and its segments are decoded in order (the chunks are queued on one HIP stream), so
// what a stream carries from chunk to chunk -- the samples before the segment, its result so far
// -- is read and written by that one segment with no atomics.
#pragma once
#include <stdint.h>

#include <vector>

#include "fg_crc.hpp"

namespace fg {
namespace streams {

struct StreamResult {  // = flacgpu_stream_result
    uint64_t n_frames, n_samples;
    uint32_t index_status, bad_frames, first_bad_frame, first_bad_status;
};
static_assert(sizeof(StreamResult) == 32, "StreamResult layout");

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Segment {
    uint32_t stream;  // whose frames
    uint32_t first;   // first frame of the segment in its chunk
    uint32_t count;   // > 0
    uint32_t frame0;  // frames of the stream before the segment
    uint64_t packed;  // the segment's first entry in the packed frame table (= chunk * max_frames + first)
};
static_assert(sizeof(Segment) == 24, "Segment layout");

// An offset k_dec_recon's capacity check (off > cap || nb > cap - off) refuses whatever the cap:
// the first comparison is true, and nothing is added to the offset before it.
constexpr uint64_t kRefuse = ~0ull;

// The PCM byte offset of a frame of `block` samples with samples_before samples of its stream
// before it (earlier chunks and earlier frames of this one; a damaged frame whose header parsed
// counts its block, one whose header did not counts 0: the rule of the one-stream scan), in a
// region of cap bytes at `base`.  A frame whose bytes would pass the region is refused.
FG_HD uint64_t frame_pcm_offset(uint64_t base, uint64_t cap, uint64_t samples_before, uint32_t block, uint32_t per) {
    const uint64_t rel = samples_before * per, nb = (uint64_t)block * per;
    return (rel > cap || nb > cap - rel) ? kRefuse : base + rel;
}

// What a run of frames adds to its stream's result.
struct Fold {
    uint64_t samples = 0;       // of the frames with status 0
    uint32_t bad = 0;           // frames with another status
    uint32_t first_bad = kNone; // the first of them, counted from the segment's first frame
    uint32_t first_status = 0;
};
FG_HD void fold_frame(Fold &f, uint32_t i, uint32_t status, uint32_t block) {
    if (status == 0) {
        f.samples += block;
        return;
    }
    f.bad += 1u;
    if (i < f.first_bad) {
        f.first_bad = i;
        f.first_status = status;
    }
}
FG_HD void fold_merge(Fold &a, const Fold &b) {
    a.samples += b.samples;
    a.bad += b.bad;
    if (b.first_bad < a.first_bad) {
        a.first_bad = b.first_bad;
        a.first_status = b.first_status;
    }
}
// the segment's fold into the stream's result; frame0: the stream's frames before the segment
FG_HD void fold_into(StreamResult &r, const Fold &f, uint32_t frame0) {
    r.n_samples += f.samples;
    r.bad_frames += f.bad;
    if (r.first_bad_frame == kNone && f.first_bad != kNone) {
        r.first_bad_frame = frame0 + f.first_bad;
        r.first_bad_status = f.first_status;
    }
}

// The segment table of a call (host): frames[s] frames of stream s (0: the stream decodes
// nothing), chunks of at most max_frames > 0.  chunk_seg[k] .. chunk_seg[k + 1]: chunk k's
// segments; its frame count is the sum of their counts (max_frames but for the last chunk).
inline void cut_segments(const std::vector<uint64_t> &frames, uint32_t max_frames, std::vector<Segment> &segs,
                         std::vector<uint32_t> &chunk_seg) {
    segs.clear();
    chunk_seg.assign(1, 0u);
    uint64_t chunk = 0;
    uint32_t fill = 0;  // frames in the open chunk
    for (size_t s = 0; s < frames.size(); s++) {
        for (uint64_t done = 0; done < frames[s];) {
            if (fill == max_frames) {
                chunk_seg.push_back((uint32_t)segs.size());
                chunk++;
                fill = 0;
            }
            const uint64_t left = frames[s] - done, room = max_frames - fill;
            const uint32_t n = (uint32_t)(left < room ? left : room);
            segs.push_back({(uint32_t)s, fill, n, (uint32_t)done, chunk * max_frames + fill});
            fill += n;
            done += n;
        }
    }
    if (segs.empty()) chunk_seg.clear();  // no chunk at all
    else chunk_seg.push_back((uint32_t)segs.size());
}

}  // namespace streams
}  // namespace fg
