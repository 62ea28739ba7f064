"""The One-Euro rule of csrc/smooth.hip (include/dir_hip.h, "temporal smoothing") restated in float64 numpy: usable / initialise / gap /
update / jitter, over the segments of a row.  tests/test_smooth_ref.py checks it against closed forms and against a literal transcription
of the paper's pseudo-code; tests/test_gpu_smooth.py checks the kernel against it.

    ref = OneEuroRef([(n_points, dims, speed_scale), ...], batch, fps=30, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, max_gap=None)
    y, updated = ref.step(x [B,F], valid [B] or None)          # B <= batch: the first B rows of the state
    ref.jitter                                                 # float64 [batch,S,2] sums (raw, filtered); ref.count int [batch]
"""
import numpy as np


def alpha(fc, dt):
    return 1.0 / (1.0 + 1.0 / (2.0 * np.pi * fc * dt))


class OneEuroRef(object):
    def __init__(self, segments, batch, fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, max_gap=None):
        self.segments = [(int(n), int(d), float(s)) for n, d, s in segments]
        self.F = sum(n * d for n, d, _ in self.segments)
        self.fps, self.min_cutoff, self.beta, self.d_cutoff = float(fps), float(min_cutoff), float(beta), float(d_cutoff)
        self.max_gap = int(round(self.fps)) if max_gap is None else int(max_gap)
        B, S = int(batch), len(self.segments)
        self.y1, self.y2, self.x1, self.x2, self.dxhat = (np.zeros((B, self.F)) for _ in range(5))
        self.age, self.run, self.count = (np.zeros(B, np.int64) for _ in range(3))
        self.jitter = np.zeros((B, S, 2))

    def slices(self):
        """-> per segment (start, n_points, dims, speed_scale)"""
        out, at = [], 0
        for n, d, s in self.segments:
            out.append((at, n, d, s))
            at += n * d
        return out

    def step(self, x, valid=None):
        x = np.asarray(x)
        xd = x.astype(np.float64)
        B = xd.shape[0]
        assert xd.shape == (B, self.F) and B <= self.age.shape[0]
        y, updated = xd.copy(), np.zeros(B, np.int32)
        for b in range(B):
            usable = (valid is None or valid[b] != 0) and bool(np.isfinite(xd[b]).all())
            if not usable:
                if self.age[b] > 0:
                    self.age[b] += 1
                self.run[b] = 0
                continue
            if self.age[b] == 0 or self.age[b] > self.max_gap:
                self.dxhat[b] = 0.0
                self.run[b], updated[b] = 1, 2
            else:
                dt = self.age[b] / self.fps
                dx = (xd[b] - self.y1[b]) / dt
                self.dxhat[b] += alpha(self.d_cutoff, dt) * (dx - self.dxhat[b])
                for at, n, d, scale in self.slices():
                    sl = slice(at, at + n * d)
                    v = scale * np.sqrt((self.dxhat[b, sl].reshape(n, d) ** 2).sum(1))
                    a = np.repeat(alpha(self.min_cutoff + self.beta * v, dt), d)
                    y[b, sl] = self.y1[b, sl] + a * (xd[b, sl] - self.y1[b, sl])
                self.run[b] += 1
                updated[b] = 1
            self.age[b] = 1
            if self.run[b] >= 3:
                for s, (at, n, d, _) in enumerate(self.slices()):
                    sl = slice(at, at + n * d)
                    self.jitter[b, s, 0] += np.sqrt(((xd[b, sl] - 2 * self.x1[b, sl] + self.x2[b, sl]).reshape(n, d) ** 2).sum(1)).sum()
                    self.jitter[b, s, 1] += np.sqrt(((y[b, sl] - 2 * self.y1[b, sl] + self.y2[b, sl]).reshape(n, d) ** 2).sum(1)).sum()
                self.count[b] += 1
            self.x2[b], self.x1[b] = self.x1[b], xd[b]
            self.y2[b], self.y1[b] = self.y1[b], y[b]
        return y, updated

    def mean_jitter(self):
        """-> float64 [batch,S,2]: mean second difference per point per frame (NaN where no frame was counted)"""
        n = np.array([s[0] for s in self.segments], np.float64)[None, :, None]
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.jitter / n / self.count[:, None, None].astype(np.float64)
