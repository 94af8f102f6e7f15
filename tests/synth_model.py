"""An independent model of the synthesizer's CONTROL rate in float64, written from the reference (rustysynth_fork/src: voice.rs,
volume_envelope.rs, modulation_envelope.rs, lfo.rs, oscillator.rs, bi_quad_filter.rs:51-75, region_pair.rs, region_ex.rs, channel.rs,
voice_collection.rs, synthesizer.rs:176-304 and 363-391, midifile_sequencer.rs:52-104), not from the product's C++.

Every quantity the reference keeps in f32 is kept in float64 here, so VALUES differ from the product's by f32 rounding, and the tests
compare them under bounds; DECISIONS (which voice object sounds in which block and in which order, the volume envelope's stage, the
looping flag, the snapshots) must be the product's exactly.  A decision is only comparable where no threshold lies within rounding
of the value compared: `Model.margins` collects the relative distance of every such comparison, and the tests assert that all are
above 1e-6 — over every block of every case, so that no case is excused.  Integers (channel state, positions) are exact."""
import math

NON_AUDIBLE = 1.0e-3
LOG_NON_AUDIBLE = -6.9077554
BLOCK = 64
FRAC = 24
DELAY, ATTACK, HOLD, DECAY, RELEASE = range(5)


def i16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


class Channel:
    def __init__(self, percussion):
        self.percussion = percussion
        self.reset()

    def reset(self):
        self.bank = 128 if self.percussion else 0
        self.patch = 0
        self.modulation = 0
        self.volume = 100 << 7
        self.pan = 64 << 7
        self.expression = 127 << 7
        self.hold = False
        self.rpn = -1
        self.pbr = 2 << 7
        self.coarse_tune = 0
        self.fine_tune = 8192
        self.pitch_bend = 0.0

    def reset_all_controllers(self):
        self.modulation = 0
        self.expression = 127 << 7
        self.hold = False
        self.rpn = -1
        self.pitch_bend = 0.0

    @staticmethod
    def coarse(cur, v):
        return i16((cur & 0x7F) | i16(v << 7))

    @staticmethod
    def fine(cur, v):
        return i16((cur & 0xFF80) | v)


class Env:
    """VolumeEnvelope (volume=True) / ModulationEnvelope"""

    def __init__(self, model, volume):
        self.m, self.volume = model, volume

    def start(self, delay, attack, hold, decay, sustain, release):
        self.attack, self.decay, self.release_t = attack, decay, release
        self.t_attack = delay
        self.t_hold = delay + attack
        self.t_decay = self.t_hold + hold
        self.t_decay_end = self.t_decay + decay
        self.t_release = 0.0
        self.release_end = release
        self.sustain = min(max(sustain, 0.0), 1.0)
        self.release_level = 0.0
        self.count = 0
        self.stage = DELAY
        self.value = 0.0
        self.priority = 0.0
        self.r = self.m.r   # the value and the priority are f32 in the reference; the times are f64 there as here
        self.process(0)

    def release(self):
        self.stage = RELEASE
        now = self.count / self.m.sr
        self.t_release = now
        self.release_end += now
        self.release_level = self.value

    def process(self, n):
        self.count += n
        t = self.count / self.m.sr
        while self.stage <= HOLD:
            end = (self.t_attack, self.t_hold, self.t_decay)[self.stage]
            self.m.margin(t, end)
            if t < end:
                break
            self.stage += 1
        if self.stage == DELAY:
            self.value, self.priority = 0.0, 4.0
            return True
        if self.stage == ATTACK:
            self.value = self.r((1.0 / self.attack) * (t - self.t_attack))
            self.priority = self.r(3.0 + self.value)
            return True
        if self.stage == HOLD:
            self.value, self.priority = 1.0, 3.0
            return True
        if self.volume:
            if self.stage == DECAY:
                x = -9.226 / self.decay * (t - self.t_decay)
                self.m.margin(x, LOG_NON_AUDIBLE)
                self.value = max(self.r(0.0 if x < LOG_NON_AUDIBLE else math.exp(x)), self.sustain)
                self.priority = self.r(1.0 + self.value)
            else:
                x = -9.226 / self.release_t * (t - self.t_release)
                self.m.margin(x, LOG_NON_AUDIBLE)
                self.value = self.r(self.release_level * (0.0 if x < LOG_NON_AUDIBLE else math.exp(x)))
                self.priority = self.value
        else:
            if self.stage == DECAY:
                self.value = max(self.r((1.0 / self.decay) * (self.t_decay_end - t)), self.sustain)
            else:
                self.value = max(self.r(self.release_level * (1.0 / self.release_t) * (self.release_end - t)), 0.0)
        if self.volume:
            self.m.margin(self.value, NON_AUDIBLE)
        return self.value > NON_AUDIBLE


class Lfo:
    def __init__(self, model):
        self.m = model
        self.active = False
        self.value = 0.0

    def start(self, delay, frequency):
        self.m.margin(frequency, 1.0e-3)
        self.value = 0.0
        self.active = frequency > 1.0e-3
        if self.active:
            self.delay, self.period, self.count = delay, 1.0 / frequency, 0

    def process(self):
        if not self.active:
            return
        self.count += BLOCK
        t = self.count / self.m.sr
        self.m.margin(t, self.delay)
        if t < self.delay:
            self.value = 0.0
            return
        phase = math.fmod(t - self.delay, self.period) / self.period
        for edge in (0.25, 0.75):
            self.m.margin_abs(phase, edge)
        if phase < 0.25:
            self.value = self.m.r(4.0 * phase)
        elif phase < 0.75:
            self.value = self.m.r(4.0 * (0.5 - phase))
        else:
            self.value = self.m.r(4.0 * (phase - 1.0))


class Voice:
    """voice.rs, with the control part of oscillator.rs and bi_quad_filter.rs:51-75.  `r` rounds where the reference holds an f32:
    the identity in the float64 evaluation, numpy.float32 in the float32 one."""

    def __init__(self, model, ident):
        self.m, self.id = model, ident
        self.vol_env, self.mod_env = Env(model, True), Env(model, False)
        self.vib_lfo, self.mod_lfo = Lfo(model), Lfo(model)
        self.cur_l = self.cur_r = self.prev_l = self.prev_r = 0.0
        self.exclusive_class = self.channel = self.key = self.velocity = 0
        self.note_gain = 0.0
        self.voice_length = 0
        self.coef = None

    def set_filter(self, cutoff, resonance):
        r, m = self.m.r, self.m
        limit = r(r(0.499) * m.sr)
        m.margin(cutoff, limit)
        self.filter_active = cutoff < limit
        if self.filter_active:
            offset = r(1.0 - r(1.0 / r(math.sqrt(2.0))))
            q = r(resonance - r(offset / r(1.0 + r(6.0 * r(resonance - 1.0)))))
            w = r(r(r(2.0 * r(math.pi)) * cutoff) / m.sr)
            cosw, alpha = r(math.cos(w)), r(r(math.sin(w)) / r(2.0 * q))
            one_minus = r(1.0 - cosw)
            b0, b1, a0, a1, a2 = r(one_minus / 2.0), one_minus, r(1.0 + alpha), r(-2.0 * cosw), r(1.0 - alpha)
            self.coef = (r(b0 / a0), r(b1 / a0), r(b0 / a0), r(a1 / a0), r(a2 / a0))

    def start(self, pgs, ir, channel, key, velocity):
        m, r = self.m, self.m.r
        tc, hz, db2lin = m.tc, m.hz, m.db2lin
        igs, smp = ir["gs"], ir["sample"]
        g = lambda i: int(pgs[i]) + int(igs[i])
        tenth = lambda i: r(r(0.1) * g(i))
        self.exclusive_class = int(igs[57])
        self.channel, self.key, self.velocity = channel, key, velocity
        if velocity > 0:
            decibels = r(r(r(2.0 * r(20.0 * r(math.log10(r(velocity / 127.0))))) - r(r(0.4) * tenth(48))) - r(0.5 * tenth(9)))
            self.note_gain = db2lin(decibels)
        else:
            self.note_gain = 0.0
        m.margin(self.note_gain, NON_AUDIBLE)
        self.cutoff = hz(g(8))
        self.resonance = db2lin(tenth(9))
        self.vib_lfo_to_pitch, self.mod_lfo_to_pitch, self.mod_env_to_pitch = r(r(0.01) * g(6)), r(r(0.01) * g(5)), r(r(0.01) * g(7))
        self.mod_lfo_to_cutoff, self.mod_env_to_cutoff = g(10), g(11)
        self.dynamic_cutoff = self.mod_lfo_to_cutoff != 0 or self.mod_env_to_cutoff != 0
        self.mod_lfo_to_volume = tenth(13)
        m.margin(self.mod_lfo_to_volume, 0.05)
        self.dynamic_volume = self.mod_lfo_to_volume > r(0.05)
        self.instrument_pan = min(max(tenth(17), -50.0), 50.0)
        knf = lambda cents: tc(cents * (60 - key))
        self.vol_env.start(tc(g(33)), tc(g(34)), r(tc(g(35)) * knf(g(39))), r(tc(g(36)) * knf(g(40))), db2lin(-tenth(37)), max(tc(g(38)), r(0.01)))
        self.mod_env.start(tc(g(25)), r(tc(g(26)) * r((145 - velocity) / 144.0)), r(tc(g(27)) * knf(g(31))), r(tc(g(28)) * knf(g(32))),
                           r(1.0 - r(tenth(29) / 100.0)), tc(g(30)))
        self.vib_lfo.start(tc(g(23)), hz(g(24)))
        self.mod_lfo.start(tc(g(21)), hz(g(22)))
        modes = int(igs[54])
        self.loop_mode = modes if modes != 2 else 0
        off = lambda coarse, fine: 32768 * int(igs[coarse]) + int(igs[fine])
        self.start_i, self.end_i = smp[0] + off(4, 0), smp[1] + off(12, 1)
        self.start_loop, self.end_loop = smp[2] + off(45, 2), smp[3] + off(50, 3)
        self.root_key = int(igs[58]) if int(igs[58]) != -1 else smp[5]
        self.tune = r(g(51) + r(r(0.01) * (g(52) + smp[6])))
        self.pitch_change_scale = r(r(0.01) * g(56))
        self.sample_rate_ratio = r(smp[4] / m.sr)
        self.looping = self.loop_mode != 0
        self.pos_lo = self.pos_hi = self.start_i << FRAC
        self.set_filter(self.cutoff, self.resonance)
        self.smoothed_cutoff = self.cutoff
        self.state = 0
        self.voice_length = 0
        self.region = ir["index"]

    def priority(self):
        return 0.0 if self.note_gain < NON_AUDIBLE else self.vol_env.priority

    def _advance(self, pos, ratio_fp):
        """the oscillator's 64 steps on the position alone (oscillator.rs:112-176): (sounds, position)"""
        if not self.looping:
            end_fp = self.end_i << FRAC
            for t in range(BLOCK):
                if pos >= end_fp:
                    return t > 0, pos
                pos += ratio_fp
            return True, pos
        end_loop_fp, length_fp = self.end_loop << FRAC, (self.end_loop - self.start_loop) << FRAC
        for _ in range(BLOCK):
            if pos >= end_loop_fp:
                pos -= length_fp
            pos += ratio_fp
        return True, pos

    def process(self):
        m, r = self.m, self.m.r
        if self.note_gain < NON_AUDIBLE:
            return None
        ch = m.channels[self.channel]
        if self.voice_length >= m.sr // 500 and self.state == 1 and not ch.hold:
            self.vol_env.release()
            self.mod_env.release()
            if self.loop_mode == 3:
                self.looping = False
            self.state = 2
        if not self.vol_env.process(BLOCK):
            return None
        self.mod_env.process(BLOCK)
        self.vib_lfo.process()
        self.mod_lfo.process()
        modulation = r(r(50.0 / 16383.0) * ch.modulation)
        vib = r(r(r(r(0.01) * modulation) + self.vib_lfo_to_pitch) * self.vib_lfo.value)
        mod = r(r(self.mod_lfo_to_pitch * self.mod_lfo.value) + r(self.mod_env_to_pitch * self.mod_env.value))
        tune = r(ch.coarse_tune + r(r(1.0 / 8192.0) * (ch.fine_tune - 8192)))
        bend = r(r((ch.pbr >> 7) + r(r(0.01) * (ch.pbr & 0x7F))) * ch.pitch_bend)
        pitch = r(r(r(self.key + vib) + mod) + r(tune + bend))
        change = r(r(self.pitch_change_scale * r(pitch - self.root_key)) + self.tune)
        ratio = r(self.sample_rate_ratio * r(2.0 ** r(change / 12.0)))
        slack = int(8 * max(1.0, ratio)) + 1
        looping = self.looping
        ok_lo = ok_hi = True
        if self.loop_mode != 1:   # (a continuous loop never ends: its position decides nothing)
            ok_lo, self.pos_lo = self._advance(self.pos_lo, int((1 << FRAC) * ratio) - slack)
            ok_hi, self.pos_hi = self._advance(self.pos_hi, int((1 << FRAC) * ratio) + slack)
        m.decided(ok_lo == ok_hi)   # the sample's end is not within rounding of a block edge
        if not ok_lo:
            return None
        if self.dynamic_cutoff:
            cents = r(r(self.mod_lfo_to_cutoff * self.mod_lfo.value) + r(self.mod_env_to_cutoff * self.mod_env.value))
            new_cutoff = r(m.factor(cents) * self.cutoff)
            lo, hi = r(0.5 * self.smoothed_cutoff), r(2.0 * self.smoothed_cutoff)
            m.margin(new_cutoff, lo)
            m.margin(new_cutoff, hi)
            m.clamped += new_cutoff < lo or new_cutoff > hi
            self.smoothed_cutoff = min(max(new_cutoff, lo), hi)
            self.set_filter(self.smoothed_cutoff, self.resonance)
        self.prev_l, self.prev_r = self.cur_l, self.cur_r
        ve = r(r(r(1.0 / 16383.0) * ch.volume) * r(r(1.0 / 16383.0) * ch.expression))
        mix = r(r(self.note_gain * r(ve * ve)) * self.vol_env.value)
        if self.dynamic_volume:
            mix = r(mix * m.db2lin(r(self.mod_lfo_to_volume * self.mod_lfo.value)))
        pan = r(r(r(100.0 / 16383.0) * ch.pan) - 50.0)
        angle = r(r(r(math.pi) / 200.0) * r(r(pan + self.instrument_pan) + 50.0))
        half_pi = r(r(math.pi) / 2.0)
        m.margin_abs(angle, 0.0)
        m.margin_abs(angle, half_pi)
        if angle <= 0.0:
            self.cur_l, self.cur_r = mix, 0.0
        elif angle >= half_pi:
            self.cur_l, self.cur_r = 0.0, mix
        else:
            self.cur_l, self.cur_r = r(mix * r(math.cos(angle))), r(mix * r(math.sin(angle)))
        if self.voice_length == 0:
            self.prev_l, self.prev_r = self.cur_l, self.cur_r
        self.voice_length += BLOCK
        mv = m.master_volume
        return dict(voice=self.id, key=self.key, stage=self.vol_env.stage, looping=looping, filter=self.filter_active, ratio=ratio, coef=self.coef,
                    gain=(r(mv * self.prev_l), r(mv * self.cur_l), r(mv * self.prev_r), r(mv * self.cur_r)), mix=mix, region=self.region)


class Model:
    def __init__(self, bank, sample_rate, polyphony, float32=False):
        """bank: the dict of synth_cases.bank_arrays().  float32: round wherever the reference holds an f32 (numpy.float32, libm
        functions taken in float64 and rounded once); otherwise every value stays float64."""
        import numpy as np
        self.r = (lambda x: float(np.float32(x))) if float32 else (lambda x: x)
        self.sr = sample_rate
        self.master_volume = 0.5
        self.margins = []      # relative distance of every compared value from its threshold
        self.undecided = 0     # decisions that rounding could turn
        self.clamped = 0       # blocks whose cutoff hit the x0.5 / x2 clamp
        self.steals = 0
        self.reuses = 0
        self.channels = [Channel(i == 9) for i in range(16)]
        self.voices = [Voice(self, i) for i in range(polyphony)]
        self.active = 0
        self.time = 0.0
        self.msg = 0
        gs, smp_idx = bank["instrument_regions"]
        self.iregions = [dict(gs=gs[i], sample=[int(x) for x in bank["samples"][int(smp_idx[i])]], index=i) for i in range(len(smp_idx))]
        self.instruments = [(int(a), int(b)) for a, b in bank["instruments"]]
        pgs, pins = bank["preset_regions"]
        self.pregions = [(pgs[i], int(pins[i])) for i in range(len(pins))]
        self.presets = [tuple(int(x) for x in p) for p in bank["presets"]]
        self.lookup = {}
        self.default, best = 0, None
        for i, (bk, patch, _, _) in enumerate(self.presets):
            pid = (bk << 16) | patch
            self.lookup[pid] = i
            if best is None or pid < best:
                self.default, best = i, pid

    def factor(self, x):   # cents_to_multiplying_factor = timecents_to_seconds (soundfont_math.rs:32-42)
        r = self.r
        return r(2.0 ** r(r(1.0 / 1200.0) * x))

    tc = factor

    def hz(self, x):       # cents_to_hertz
        return self.r(self.r(8.176) * self.factor(x))

    def db2lin(self, x):   # decibels_to_linear
        r = self.r
        return r(10.0 ** r(r(0.05) * x))

    def margin(self, value, threshold):
        scale = max(abs(value), abs(threshold))
        self.margins.append(abs(value - threshold) / scale if scale > 0 else 1.0)

    def margin_abs(self, value, threshold):
        self.margins.append(abs(value - threshold) if value != threshold else 1.0)

    def decided(self, ok):
        self.undecided += not ok

    @staticmethod
    def contains(gs, key, vel):
        kr, vr = int(gs[43]), int(gs[44])
        return (kr & 0xFF) <= key <= ((kr >> 8) & 0xFF) and (vr & 0xFF) <= vel <= ((vr >> 8) & 0xFF)

    def request_new(self, igs, channel):
        ec = int(igs[57])
        if ec != 0:
            for i in range(self.active):
                if self.voices[i].exclusive_class == ec and self.voices[i].channel == channel:
                    self.reuses += 1
                    return self.voices[i]
        if self.active < len(self.voices):
            self.active += 1
            return self.voices[self.active - 1]
        cand, lowest = 0, float("inf")
        prios = [self.voices[i].priority() for i in range(self.active)]
        for i, p in enumerate(prios):
            if p < lowest:
                lowest, cand = p, i
            elif p == lowest and self.voices[i].voice_length > self.voices[cand].voice_length:
                cand = i
        for i, p in enumerate(prios):   # no other voice's priority is within rounding of the stolen one's, unless it is the same number
            if p != lowest:
                self.margin(p, lowest)
        self.steals += 1
        return self.voices[cand]

    def note_off(self, channel, key):
        for v in self.voices[:self.active]:
            if v.channel == channel and v.key == key and v.state == 0:
                v.state = 1

    def note_on(self, channel, key, vel):
        if vel == 0:
            return self.note_off(channel, key)
        ch = self.channels[channel]
        pid = (ch.bank << 16) | ch.patch
        preset = self.default
        if pid in self.lookup:
            preset = self.lookup[pid]
        else:
            gm = ch.patch if ch.bank < 128 else 128 << 16
            preset = self.lookup.get(gm, preset)
        _, _, first, count = self.presets[preset]
        for pgs, inst in self.pregions[first:first + count]:
            if not self.contains(pgs, key, vel):
                continue
            i0, n = self.instruments[inst]
            for ir in self.iregions[i0:i0 + n]:
                if self.contains(ir["gs"], key, vel):
                    self.request_new(ir["gs"], channel).start(pgs, ir, channel, key, vel)

    def message(self, channel, command, d1, d2):
        if not 0 <= channel < 16:
            return
        c = self.channels[channel]
        if command == 0x80:
            self.note_off(channel, d1)
        elif command == 0x90:
            self.note_on(channel, d1, d2)
        elif command == 0xB0:
            if d1 == 0x00:
                c.bank = d2 + (128 if c.percussion else 0)
            elif d1 == 0x01:
                c.modulation = Channel.coarse(c.modulation, d2)
            elif d1 == 0x21:
                c.modulation = Channel.fine(c.modulation, d2)
            elif d1 == 0x06:
                if c.rpn == 0:
                    c.pbr = Channel.coarse(c.pbr, d2)
                elif c.rpn == 1:
                    c.fine_tune = Channel.coarse(c.fine_tune, d2)
                elif c.rpn == 2:
                    c.coarse_tune = i16(d2 - 64)
            elif d1 == 0x26:
                if c.rpn == 0:
                    c.pbr = Channel.fine(c.pbr, d2)
                elif c.rpn == 1:
                    c.fine_tune = Channel.fine(c.fine_tune, d2)
            elif d1 == 0x07:
                c.volume = Channel.coarse(c.volume, d2)
            elif d1 == 0x27:
                c.volume = Channel.fine(c.volume, d2)
            elif d1 == 0x0A:
                c.pan = Channel.coarse(c.pan, d2)
            elif d1 == 0x2A:
                c.pan = Channel.fine(c.pan, d2)
            elif d1 == 0x0B:
                c.expression = Channel.coarse(c.expression, d2)
            elif d1 == 0x2B:
                c.expression = Channel.fine(c.expression, d2)
            elif d1 == 0x40:
                c.hold = d2 >= 64
            elif d1 == 0x65:
                c.rpn = Channel.coarse(c.rpn, d2)
            elif d1 == 0x64:
                c.rpn = Channel.fine(c.rpn, d2)
            elif d1 == 0x78:
                for v in self.voices[:self.active]:
                    if v.channel == channel:
                        v.note_gain = 0.0
            elif d1 == 0x79:
                c.reset_all_controllers()
            elif d1 == 0x7B:
                for v in self.voices[:self.active]:
                    if v.channel == channel and v.state == 0:
                        v.state = 1
        elif command == 0xC0:
            c.patch = d1
        elif command == 0xE0:
            c.pitch_bend = self.r(self.r(1.0 / 8192.0) * ((d1 | (d2 << 7)) - 8192))

    def run(self, events, n_blocks, snapshot_blocks=()):
        """-> (blocks: per block the list of record dicts in active-list order, snapshots: per snapshot block [(key, left, right)])"""
        t, chs, cmds, d1s, d2s = events
        blocks, snaps = [], []
        dt = BLOCK / self.sr
        for b in range(n_blocks):
            while self.msg < len(t) and t[self.msg] <= self.time:
                i = self.msg
                self.msg += 1
                self.message(int(chs[i]), int(cmds[i]), int(d1s[i]), int(d2s[i]))
            self.time += dt   # (the same f64 additions as the reference's: the event rule needs no margin)
            recs, i = [], 0
            while i != self.active:
                r = self.voices[i].process()
                if r is not None:
                    recs.append(r)
                    i += 1
                else:
                    self.active -= 1
                    self.voices[i], self.voices[self.active] = self.voices[self.active], self.voices[i]
            blocks.append(recs)
            if b in snapshot_blocks:
                snaps.append([(v.key, v.cur_l, v.cur_r) for v in self.voices[:self.active]])
        return blocks, snaps
