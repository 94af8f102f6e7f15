// panels_host.hpp — the three meshes of the viewer's DisplayMode::Debugging for ONE stream on the host: the spectrum line with its
// peak discs (update_spectrum, update.rs:474-638), the calmness histogram (update_calmness_histogram, :744-869) and the scene
// calmness graph with its history ring (update_scene_calmness_graph, :640-742; SceneCalmnessHistory, mod.rs:114-133).  The
// one-stream face and second reference of PanelsBatch (panels_batch.hpp); the arithmetic is panels_math.hpp's on both.
//
// A mesh is positions [vertices][3] and colours [vertices][4]; what depends on the counts alone — indices, UVs, the normal (0, 0, 1)
// of every vertex — comes from panel_topology.  The reference's transforms (the histogram's y flip, the placement relative to the
// camera), the visibility toggles and the concatenation of line and discs into one mesh stay with the caller.
#pragma once

#include <cstdint>
#include <vector>

#include "panels_math.hpp"

namespace pvq {

// update.rs:560-569 for every i % bpo: calculate_color(bpo, (k as f32 + 0.5 + (bpo - 3 (bpo / 12)) as f32) % bpo as f32, colors,
// gray_level, 10.0).  Every term is exact in f32 below 2^23, so bucket i's colour is entry i % bpo.  rgb [bpo][3]; colors null: COLORS.
void panel_color_table(uint32_t buckets_per_octave, const float* colors, float gray_level, float* rgb);
// update.rs:447-449: (cos a_i, sin a_i) of a_i = (i as f32 / 12.0) * TAU, each the double function rounded once.  cs [12][2].
void panel_disc_table(float* cs);

// update_spectrum.  rgb_table / cs: the two tables above.  line_pos [4 (n - 1)][3], line_rgba [4 (n - 1)][4], disc_pos
// [n_peaks][13][3], disc_rgba [n_peaks][13][4]; any may be null.  n_buckets >= 2.
void spectrum_mesh(uint32_t n_buckets, uint32_t buckets_per_octave, const float* x_vqt_smoothed, const float* center, const float* size,
                   uint32_t n_peaks, const float* rgb_table, const float* cs, float* line_pos, float* line_rgba, float* disc_pos,
                   float* disc_rgba);
// update_calmness_histogram.  pos [4 (n - 1)][3], rgba [4 (n - 1)][4]; either may be null.  n_buckets >= 2.
void calmness_histogram_mesh(uint32_t n_buckets, const float* calmness, float* pos, float* rgba);

// update_scene_calmness_graph's ring and mesh
class CalmnessGraph {
   public:
    explicit CalmnessGraph(uint32_t capacity) : values_(capacity, 0.0f) {}
    uint32_t capacity() const { return static_cast<uint32_t>(values_.size()); }
    void push(float value) {   // update.rs:656-658
        values_[write_index_] = value;
        write_index_ = (write_index_ + 1u) % capacity();
    }
    // the last `capacity` pushed values, oldest first, zeros where nothing has been pushed: the ring from write_index (update.rs:662-666)
    void history(float* out) const;
    // update.rs:661-718.  pos [4 (capacity - 1)][3], rgba [4 (capacity - 1)][4]; either may be null
    void mesh(float* pos, float* rgba) const;

   private:
    std::vector<float> values_;
    uint32_t write_index_ = 0;
};

// n_quads quads followed by n_circles discs.  indices [6 n_quads + 36 n_circles]: a quad with base b gives b+2, b+1, b, b+2, b, b+3
// (update.rs:543-549), a disc with base b the triangles (b, b+1+i, b+1+(i+1)%12) (update.rs:458-463).  uvs [4 n_quads + 13
// n_circles][2]: (0,1), (0,0), (1,0), (1,1) per quad (update.rs:551-554); (0.5, 0.5), then (0.5 + 0.5 cos a_i, 0.5 + 0.5 sin a_i)
// per disc (update.rs:442, :454).  Either may be null.
void panel_topology(uint32_t n_quads, uint32_t n_circles, uint32_t* indices, float* uvs);

}  // namespace pvq
