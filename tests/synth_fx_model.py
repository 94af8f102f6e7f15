"""The synthesizer's effects in NumPy, written from rustysynth_fork/src/reverb.rs, chorus.rs and synthesizer.rs:393-475: float32 where
the reference computes in f32, float64 where it computes in f64, no fused operations (NumPy has none).  The effects advance ONE SAMPLE
AT A TIME — never a block at a time — so the model does not share the kernel's argument about what is parallel within a block; a
sample's work is vectorised across the 16 combs and across the two channels, which the reference keeps independent.

The model is fed with the host's plan, sends and delay table, as the audio-rate check of tests/test_synth.py is fed with the plan."""
import numpy as np

f32 = np.float32
FLUSH = f32(1.0e-6)
NON_AUDIBLE = f32(1.0e-3)
COMB = [1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617]   # reverb.rs:35-50
ALLPASS = [556, 441, 341, 225]                            # reverb.rs:51-58
SPREAD = 23


def lengths(sr):
    """(comb lengths [2][8], all-pass lengths [2][4], chorus ring length, delay table length)"""
    scale = lambda tuning: int(np.floor(sr / 44100.0 * tuning + 0.5))   # f64 round (no length lies on a half here)
    comb = np.array([[scale(t + c * SPREAD) for t in COMB] for c in range(2)])
    allpass = np.array([[scale(t + c * SPREAD) for t in ALLPASS] for c in range(2)])
    return comb, allpass, int(sr * (0.002 + 0.0019)) + 2, int(np.floor(sr / 0.4 + 0.5))


def delay_table(sr):
    """chorus.rs:24-29 with NumPy's sin (libm's may differ in the last f64 bit: compare within one f32 unit in the last place)"""
    n = lengths(sr)[3]
    phase = 2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n)
    return (float(sr) * (0.002 + 0.0019 * np.sin(phase))).astype(f32)


def reverb_constants():
    """Reverb::new's setters in float32 (reverb.rs:121-124, 195-236): feedback, damp1, damp2, wet1, wet2"""
    wet = (f32(1.0) / f32(3.0)) * f32(3.0)
    room = f32(0.5) * f32(0.28) + f32(0.7)
    damp = f32(0.5) * f32(0.4)
    width = f32(1.0)
    return room, damp, f32(1.0) - damp, wet * (width / f32(2.0) + f32(0.5)), wet * ((f32(1.0) - width) / f32(2.0))


class Effects:
    """Chorus + Reverb, one sample at a time"""

    def __init__(self, sr, table):
        comb, allpass, self.ring_len, table_len = lengths(sr)
        assert table.dtype == f32 and table.size == table_len
        self.table = table.astype(np.float64)
        self.comb_len, self.ap_len = comb.reshape(16), allpass   # comb c * 8 + i
        self.comb = np.zeros((16, int(comb.max())), f32)
        self.ap = np.zeros((2, 4, int(allpass.max())), f32)
        self.store = np.zeros(16, f32)
        self.ring = np.zeros((2, self.ring_len), f32)
        self.count = 0
        self.feedback, self.damp1, self.damp2, self.wet1, self.wet2 = reverb_constants()
        self.flushed = dict(comb=0, store=0, allpass=0)   # flushes of a value that was not already zero
        self._i16, self._i2 = np.arange(16), np.arange(2)

    def sample(self, cin, rin):
        """cin: float32 [2] (chorus input left, right), rin: float32 scalar -> (chorus out [2], reverb out [2])"""
        n, two = self.count, self._i2
        # chorus.rs:59-117
        ri = n % self.ring_len
        ti = np.array([n % self.table.size, (n + self.table.size // 4) % self.table.size])
        position = np.float64(ri) - self.table[ti]
        position = np.where(position < 0.0, position + float(self.ring_len), position)
        i1 = position.astype(np.int64)
        i2 = np.where(i1 + 1 == self.ring_len, 0, i1 + 1)
        x1, x2 = self.ring[two, i1].astype(np.float64), self.ring[two, i2].astype(np.float64)
        cout = (x1 + (position - i1.astype(np.float64)) * (x2 - x1)).astype(f32)
        self.ring[:, ri] = cin
        # reverb.rs:272-314: the 16 combs
        ci = n % self.comb_len
        v = self.comb[self._i16, ci]
        small = np.abs(v) < FLUSH
        self.flushed["comb"] += int(np.count_nonzero(small & (v != 0)))
        out = np.where(small, f32(0), v)
        store = out * self.damp2 + self.store * self.damp1
        small = np.abs(store) < FLUSH
        self.flushed["store"] += int(np.count_nonzero(small & (store != 0)))
        self.store = np.where(small, f32(0), store)
        self.comb[self._i16, ci] = rin + self.store * self.feedback
        o = out.reshape(2, 8)
        x = np.zeros(2, f32)
        for i in range(8):   # output_block += output, comb 1 .. 8 onto 0
            x = x + o[:, i]
        # reverb.rs:351-383: four all-passes in series
        for k in range(4):
            ai = n % self.ap_len[:, k]
            bufout = self.ap[two, k, ai]
            small = np.abs(bufout) < FLUSH
            self.flushed["allpass"] += int(np.count_nonzero(small & (bufout != 0)))
            bufout = np.where(small, f32(0), bufout)
            self.ap[two, k, ai] = x + bufout * f32(0.5)
            x = bufout - x
        if f32(1.0) - self.wet1 > f32(1.0e-3) or self.wet2 > f32(1.0e-3):   # reverb.rs:185
            x = np.array([x[0] * self.wet1 + x[1] * self.wet2, x[1] * self.wet1 + x[0] * self.wet2], f32)
        self.count = n + 1
        return cout, x

    def process(self, cin_l, cin_r, rin):
        n = cin_l.size
        cout, rout = np.zeros((2, n), f32), np.zeros((2, n), f32)
        cin = np.stack([cin_l, cin_r], axis=1).astype(f32)
        for t in range(n):
            c, r = self.sample(cin[t], f32(rin[t]))
            cout[:, t], rout[:, t] = c, r
        return cout[0], cout[1], rout[0], rout[1]


def voice_blocks(arrays, ptr, rec, n_blocks):
    """per block the [n_records][64] float32 samples of its voices after oscillator and filter (oscillator.rs:112-176,
    bi_quad_filter.rs:77-99): the records of a block are independent voices, walked sample by sample over vectors of them"""
    wave = arrays["wave_data"].astype(np.int64)
    gs, smp_idx = arrays["instrument_regions"]
    desc = np.zeros((len(smp_idx), 4), np.int64)
    for i in range(len(smp_idx)):
        s, g = arrays["samples"][int(smp_idx[i])].astype(np.int64), gs[i].astype(np.int64)
        desc[i] = (s[0] + 32768 * g[4] + g[0], s[1] + 32768 * g[12] + g[1], s[2] + 32768 * g[45] + g[2], s[3] + 32768 * g[50] + g[3])
    pos, mem, lane_desc = np.zeros(64, np.int64), np.zeros((64, 4), f32), np.zeros(64, np.int64)
    fp_to_sample = f32(1.0) / f32(32768 * (1 << 24))
    for b in range(n_blocks):
        r = rec[ptr[b]:ptr[b + 1]]
        n = r.size
        if n == 0:
            yield np.zeros((0, 64), f32)
            continue
        v = r["voice"].astype(np.int64)
        started = (r["flags"] & 1) != 0
        lane_desc[v[started]] = r["desc"][started]
        d = desc[lane_desc[v]]
        p = np.where(started, d[:, 0] << 24, pos[v])
        x1, x2, y1, y2 = (np.where(started, f32(0), mem[v, k]) for k in range(4))
        looping, active = (r["flags"] & 2) != 0, (r["flags"] & 4) != 0
        ratio = (r["ratio_hi"].astype(np.int64) << 32) | r["ratio_lo"].astype(np.int64)
        end_loop, length = d[:, 3], d[:, 3] - d[:, 2]
        a = r["a"]
        block = np.zeros((n, 64), f32)
        for t in range(64):
            p = np.where(looping & (p >= (end_loop << 24)), p - (length << 24), p)
            i1 = p >> 24
            live = looping | (i1 < d[:, 1])
            i2 = np.where(looping & (i1 + 1 >= end_loop), i1 + 1 - length, i1 + 1)
            w1, w2 = wave[np.where(live, i1, 0)], wave[np.where(live, i2, 0)]
            x = fp_to_sample * np.where(live, (w1 << 24) + (p & ((1 << 24) - 1)) * (w2 - w1), 0).astype(f32)
            p = np.where(live, p + ratio, p)
            y = a[:, 0] * x + a[:, 1] * x1 + a[:, 2] * x2 - a[:, 3] * y1 - a[:, 4] * y2
            out = np.where(active, y, x).astype(f32)
            x2, x1, y2, y1 = np.where(active, x1, x2), np.where(active, x, x1), np.where(active, y1, y2), np.where(active, y, y1)
            block[:, t] = out
        ina = ~active   # bi_quad_filter.rs:93-98
        x2, x1 = np.where(ina, block[:, 62], x2), np.where(ina, block[:, 63], x1)
        y2, y1 = np.where(ina, x2, y2), np.where(ina, x1, y1)
        pos[v] = p
        mem[v] = np.stack([x1, x2, y1, y2], axis=1)
        yield block


def write_block(dst, prev, cur, source, branches=None):
    """synthesizer.rs:478-495 with array_math.rs:8-24"""
    prev, cur = f32(prev), f32(cur)
    if max(prev, cur) < NON_AUDIBLE:
        branch = "skip"
    elif abs(cur - prev) < f32(1.0e-3):
        branch = "constant"
        dst += cur * source
    else:
        branch = "slope"
        step = f32(1.0 / 64.0) * (cur - prev)
        g, acc = np.empty(64, f32), prev
        for t in range(64):
            g[t] = acc
            acc = f32(acc + step)
        dst += g * source
    if branches is not None:
        branches[branch] = branches.get(branch, 0) + 1


def render(arrays, sr, ptr, rec, sends, table, n_blocks, master_volume=0.5):
    """synthesizer.rs:363-476 with effects on: dict(left, right, chorus_in [2], reverb_in, chorus_out [2], reverb_out [2], flushed,
    branches = how often each write_block branch was taken by the chorus and by the reverb sums)"""
    fx = Effects(sr, table)
    mv = f32(master_volume)
    n = n_blocks * 64
    out = dict(left=np.zeros(n, f32), right=np.zeros(n, f32), chorus_in=np.zeros((2, n), f32), reverb_in=np.zeros(n, f32),
               chorus_out=np.zeros((2, n), f32), reverb_out=np.zeros((2, n), f32), branches=dict(chorus={}, reverb={}))
    for b, block in enumerate(voice_blocks(arrays, ptr, rec, n_blocks)):
        sl = slice(b * 64, (b + 1) * 64)
        r, s = rec[ptr[b]:ptr[b + 1]], sends[ptr[b]:ptr[b + 1]]
        dry = np.zeros((2, 64), f32)
        cin, rin = out["chorus_in"][:, sl], out["reverb_in"][sl]
        for k in range(r.size):   # record order is the order of every sum
            write_block(dry[0], r["gain"][k, 0], r["gain"][k, 1], block[k])
            write_block(dry[1], r["gain"][k, 2], r["gain"][k, 3], block[k])
        for k in range(r.size):
            write_block(cin[0], s["chorus"][k, 0], s["chorus"][k, 1], block[k], out["branches"]["chorus"])
            write_block(cin[1], s["chorus"][k, 2], s["chorus"][k, 3], block[k], out["branches"]["chorus"])
        for k in range(r.size):
            write_block(rin, s["reverb"][k, 0], s["reverb"][k, 1], block[k], out["branches"]["reverb"])
        for t in range(64):
            c, rv = fx.sample(cin[:, t], rin[t])
            out["chorus_out"][:, b * 64 + t], out["reverb_out"][:, b * 64 + t] = c, rv
        for c, name in enumerate(("left", "right")):   # array_math.rs:8-13, twice
            v = dry[c] + mv * out["chorus_out"][c, sl]
            out[name][sl] = v + mv * out["reverb_out"][c, sl]
    out["flushed"] = fx.flushed
    return out
