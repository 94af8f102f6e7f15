"""scene_model.SceneModel with the viewer's `ml` branch (pitchvis_viewer/src/display_system/update.rs:247-255 with
display_system/util.rs:23-31), written from the reference alone; it does not call the library.  A ball the frame keys becomes opaque
when the note model infers its MIDI pitch (probability > 0.35) and nearly transparent (a tenth of its alpha) when not; a bin whose
pitch lies above 127 keeps its alpha.  FREQ_A1_MIDI_KEY_ID = 33 is pitchvis_train/src/train.rs:34's (the viewer names it without
defining it)."""
import numpy as np

import scene_model as M

f32 = np.float32
FREQ_A1_MIDI_KEY_ID = 33
THRESHOLD = f32(0.35)


def midi_pitch(bpo, bin_index):
    """util.rs:23-31 in f32: round(bin / bpo * 12) + 33, None above 127"""
    m = int(M.rround(f32(f32(f32(bin_index) / f32(bpo)) * f32(12.0)))) + FREQ_A1_MIDI_KEY_ID
    return m if m <= 127 else None


class SceneMlModel(M.SceneModel):
    def update(self, peaks, calmness, accuracy, deviation, scene_calmness, dt_ns, ml_prob=None):
        super().update(peaks, calmness, accuracy, deviation, scene_calmness, dt_ns)
        if ml_prob is None or not peaks:
            return
        prob = np.asarray(ml_prob, f32)
        for idx in {M.as_usize(np.trunc(f32(c))) for c, _ in peaks}:       # the keys of update.rs:208-212's map
            if idx >= self.n:
                continue
            m = midi_pitch(self.bpo, idx)
            if m is None:
                continue
            coef = self.rgba[idx, 3]                                         # update.rs:229, as the frame just set it
            self.rgba[idx, 3] = f32(1.0) if prob[m] > THRESHOLD else f32(coef * f32(0.1))
