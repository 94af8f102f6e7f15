"""Inputs of the synth stage's tests, all generated here: a bank of a few samples of some hundred int16 values each (a single-cycle
sine loop and a quiet copy of it, a saw with LOOP_UNTIL_NOTE_OFF, a short click without a loop, a two-value loop that runs away), a handful of regions, and
event lists of 1-2 s at 22 050 Hz.  Generator values are chosen so that no envelope boundary or LFO breakpoint falls on a block time
(tests/test_synth.py asserts it over every block of every case)."""
import numpy as np

SR = 22050
BLOCK = 64
G = dict(mod_lfo_to_pitch=5, vib_lfo_to_pitch=6, mod_env_to_pitch=7, cutoff=8, q=9, mod_lfo_to_cutoff=10, mod_env_to_cutoff=11, mod_lfo_to_volume=13,
         pan=17, delay_mod_lfo=21, freq_mod_lfo=22, delay_vib_lfo=23, freq_vib_lfo=24, delay_mod_env=25, attack_mod_env=26, hold_mod_env=27,
         decay_mod_env=28, sustain_mod_env=29, release_mod_env=30, delay_vol_env=33, attack_vol_env=34, hold_vol_env=35, decay_vol_env=36,
         sustain_vol_env=37, release_vol_env=38, key_to_vol_hold=39, key_to_vol_decay=40, instrument=41, key_range=43, vel_range=44, attenuation=48,
         coarse_tune=51, fine_tune=52, sample_id=53, sample_modes=54, scale_tuning=56, exclusive_class=57, root_key=58)

SINE_N = 100   # one cycle: 220.5 Hz at its root key 57 (A3 = 220 Hz)


def _wave():
    rng = np.random.default_rng(11)
    sine = np.round(30000 * np.sin(2 * np.pi * np.arange(SINE_N + 8) / SINE_N)).astype(np.int16)          # [0, 108), loop [0, 100)
    saw = np.round(24000 * (2 * ((np.arange(200) % 50) / 50.0) - 1) * np.minimum(1, np.arange(200) / 40.0)).astype(np.int16)
    click = np.round(28000 * rng.uniform(-1, 1, 150) * np.exp(-np.arange(150) / 40.0)).astype(np.int16)
    wave = np.zeros(700, np.int16)
    wave[560:668] = np.round(sine * (8000.0 / 30000.0)).astype(np.int16)   # the same cycle, quiet: loop [560, 660)
    wave[0:108] = sine
    wave[120:320] = saw      # loop [170, 270)
    wave[330:480] = click    # zeros behind it: the guard points
    return wave


def bank_arrays():
    """the arguments of SynthBank.from_arrays"""
    from pitchvis_amd.synth import instrument_generator_defaults, preset_generator_defaults
    wave = _wave()
    # start, end, start_loop, end_loop, sample_rate, original_pitch, pitch_correction
    samples = np.array([[0, 108, 0, 100, SR, 57, 0],
                        [120, 320, 170, 270, SR, 60, 0],
                        [330, 480, 330, 330, 32000, 72, 3],
                        [0, 108, 0, 2, SR, 57, 0],
                        [560, 668, 560, 660, SR, 57, 0]], np.int32)

    def ir(sample, **kw):
        gs = instrument_generator_defaults()
        for k, v in kw.items():
            gs[G[k]] = v
        gs[G["sample_id"]] = sample
        return gs, sample

    regions = [
        ir(0, sample_modes=1, release_vol_env=-3000),                                                              # 0 sine: filter inactive, centre
        ir(1, sample_modes=3, cutoff=9000, q=60, attack_vol_env=-4100, decay_vol_env=-1100, sustain_vol_env=120, release_vol_env=-2900,
           mod_env_to_cutoff=2500, attack_mod_env=-2300, decay_mod_env=-900, sustain_mod_env=400, release_mod_env=-2500, mod_env_to_pitch=30,
           key_to_vol_decay=20, key_to_vol_hold=-10),                                                                # 1 saw
        ir(1, sample_modes=1, cutoff=12300, mod_lfo_to_cutoff=600, freq_mod_lfo=-851, delay_mod_lfo=-7000, release_vol_env=-3300,
           attenuation=60),                                                                                          # 2 sweep: the filter goes off and on
        ir(1, sample_modes=1, cutoff=8000, q=30, mod_lfo_to_cutoff=6000, freq_mod_lfo=1550, delay_mod_lfo=-7100, mod_lfo_to_volume=30,
           mod_lfo_to_pitch=40, vib_lfo_to_pitch=25, freq_vib_lfo=-500, delay_vib_lfo=-5000, release_vol_env=-3500),  # 3 wobble: the cutoff clamp
        ir(2, sample_modes=0, exclusive_class=1, release_vol_env=-2000, key_range=0x4500),                         # 4 click, keys 0 .. 69
        ir(2, sample_modes=0, exclusive_class=1, release_vol_env=-2000, key_range=0x7F46, fine_tune=-20),            # 5 click, keys 70 .. 127
        ir(0, sample_modes=1, pan=-500, release_vol_env=-3100, attenuation=30),                                      # 6 layer: sine hard left
        ir(1, sample_modes=1, pan=250, release_vol_env=-3200, vel_range=0x7F28, scale_tuning=50),                    # 7 layer: saw half right, velocity >= 40
        ir(3, sample_modes=1, coarse_tune=60),                                                                       # 8 a two-value loop, five octaves up
        ir(4, sample_modes=1, release_vol_env=-3000),                                                                # 9 the quiet sine
    ]
    instruments = np.array([[0, 1], [1, 1], [2, 1], [3, 1], [4, 2], [6, 2], [8, 1], [9, 1]], np.uint32)

    def pr(instrument, **kw):
        gs = preset_generator_defaults()
        for k, v in kw.items():
            gs[G[k]] = v
        gs[G["instrument"]] = instrument
        return gs, instrument

    pregions = [pr(0), pr(1, release_vol_env=200), pr(2), pr(3), pr(4), pr(5, attenuation=20), pr(6), pr(7)]
    presets = np.array([[0, k, k, 1] for k in range(8)], np.int32)   # bank 0, patch k
    return dict(wave_data=wave, samples=samples,
                instrument_regions=(np.stack([r[0] for r in regions]), np.array([r[1] for r in regions], np.uint32)), instruments=instruments,
                preset_regions=(np.stack([r[0] for r in pregions]), np.array([r[1] for r in pregions], np.uint32)), presets=presets)


def ev(*rows):
    """rows of (time_s, channel, command, data1, data2), sorted by time (stable)"""
    rows = sorted(rows, key=lambda r: r[0])
    a = np.array(rows, np.float64).reshape(-1, 5)
    return (a[:, 0].copy(), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.int32), a[:, 4].astype(np.int32))


ON, OFF, CC, PC, BEND = 0x90, 0x80, 0xB0, 0xC0, 0xE0


def _steal():
    rows = [(0.0, c, PC, 0 if c == 0 else 1, 0) for c in (0, 1)]
    rows += [(0.0003 + 0.004 * i, i % 2, ON, 36 + i, 40 + i) for i in range(65)]           # the 65th note needs a 65th voice
    rows += [(0.3001 + 0.0035 * i, 0, OFF, 36 + i, 0) for i in range(0, 20, 2)]   # (released one by one: no two priorities within rounding)
    rows += [(0.4, 1, ON, 50, 90), (0.4001, 0, ON, 51, 90), (0.4002, 0, ON, 52, 90)]
    return ev(*rows)


# name -> (events, n_blocks, maximum_polyphony)
CASES = {
    "sine_root": (ev((0.0, 0, ON, 57, 100), (0.8001, 0, OFF, 57, 0)), 360, 64),
    "steal": (_steal(), 200, 64),
    "exclusive": (ev((0.0, 0, PC, 4, 0), (0.0001, 0, ON, 60, 100), (0.0031, 0, ON, 75, 110), (0.0061, 0, ON, 62, 90), (0.0062, 1, PC, 4, 0),
                     (0.0063, 1, ON, 64, 90)), 120, 64),
    "hold_pedal": (ev((0.0, 0, PC, 1, 0), (0.0001, 0, ON, 60, 100), (0.1001, 0, CC, 0x40, 127), (0.2001, 0, OFF, 60, 0), (0.5001, 0, CC, 0x40, 0),
                      (0.5002, 0, ON, 64, 80), (0.5003, 0, CC, 0x7B, 0)), 350, 64),
    "pitch_bend": (ev((0.0, 0, ON, 57, 100), (0.1001, 0, BEND, 0, 96), (0.2001, 0, BEND, 127, 127), (0.2501, 0, CC, 0x65, 0), (0.2502, 0, CC, 0x64, 0),
                      (0.2503, 0, CC, 0x06, 12), (0.2504, 0, CC, 0x26, 50), (0.3001, 0, BEND, 0, 0), (0.4701, 0, CC, 0x01, 100),
                      (0.4702, 0, CC, 0x21, 7), (0.4001, 0, CC, 0x65, 0), (0.4002, 0, CC, 0x64, 2), (0.4003, 0, CC, 0x06, 70),
                      (0.4501, 0, CC, 0x64, 1), (0.4502, 0, CC, 0x06, 80), (0.4503, 0, CC, 0x26, 3), (0.5001, 0, CC, 0x79, 0)), 350, 64),
    "all_sound_off": (ev((0.0, 0, PC, 1, 0), (0.0001, 0, ON, 60, 100), (0.0002, 0, ON, 67, 100), (0.0003, 1, ON, 57, 100), (0.2001, 0, CC, 0x78, 0),
                         (0.3001, 0, ON, 62, 100)), 200, 64),
    "noloop_end": (ev((0.0, 0, PC, 4, 0), (0.0001, 0, ON, 69, 100), (0.0301, 0, ON, 100, 100), (0.0601, 0, ON, 20, 100)), 200, 64),
    "loop_until_off": (ev((0.0, 0, PC, 1, 0), (0.0001, 0, ON, 48, 100), (0.0002, 0, ON, 84, 64), (0.3001, 0, OFF, 48, 0), (0.3501, 0, OFF, 84, 0)), 350, 64),
    "sweep": (ev((0.0, 0, PC, 2, 0), (0.0001, 0, ON, 60, 110), (0.9001, 0, OFF, 60, 0)), 400, 64),
    "wobble": (ev((0.0, 0, PC, 3, 0), (0.0001, 0, ON, 55, 120), (0.0002, 0, CC, 0x01, 64), (0.9001, 0, OFF, 55, 0)), 400, 64),
    "gains": (ev((0.0, 0, PC, 5, 0), (0.0001, 0, ON, 57, 100), (0.0002, 0, ON, 64, 30), (0.1001, 0, CC, 0x07, 30), (0.1501, 0, CC, 0x27, 90),
                 (0.2001, 0, CC, 0x0B, 64), (0.2501, 0, CC, 0x2B, 11), (0.3001, 0, CC, 0x0A, 0), (0.3501, 0, CC, 0x0A, 127), (0.3801, 0, CC, 0x2A, 127),
                 (0.4001, 0, CC, 0x07, 0), (0.4501, 0, CC, 0x07, 127), (0.5001, 0, CC, 0x5B, 10), (0.5002, 0, CC, 0x5D, 20), (0.5003, 0, CC, 0x00, 1),
                 (0.6001, 0, OFF, 57, 0)), 300, 8),
    "mixed": (ev((0.0, 0, PC, 0, 0), (0.0, 1, PC, 1, 0), (0.0, 2, PC, 2, 0), (0.0, 3, PC, 3, 0), (0.0, 4, PC, 5, 0), (0.0, 9, PC, 4, 0), (0.0, 20, ON, 60, 100),
                 *[(0.0101 + 0.03 * i, i % 5, ON, 40 + 3 * i, 50 + 5 * i) for i in range(16)],
                 *[(0.2101 + 0.03 * i, i % 5, OFF, 40 + 3 * i, 0) for i in range(16)],
                 *[(0.0151 + 0.05 * i, 9, ON, 50 + i, 100) for i in range(12)]), 340, 16),
    "silence": (ev(), 40, 64),
}
ONE_NOTE = ev((0.0, 0, PC, 7, 0), (0.0, 0, CC, 0x07, 127), (0.0, 0, ON, 57, 127))   # the quiet sine, as loud as the channel goes
RUNAWAY = (ev((0.0, 0, PC, 6, 0), (0.0301, 0, ON, 100, 100)), 30, 64)   # block 11 would read outside wave_data


def chunked(events, n_blocks, cuts):
    """the calls of a render split at `cuts` (block numbers): [(events, n_blocks_of_the_call)]"""
    edges = [0] + list(cuts) + [n_blocks]
    return [(events, edges[i + 1] - edges[i]) for i in range(len(edges) - 1)]
