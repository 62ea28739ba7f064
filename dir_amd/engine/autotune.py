"""Per-layer kernel choice: the two autotuners and the tuning tables (the part of DirEngine that picks DIR_CONV_VARIANT codes)."""
import json
import os

import torch

from .. import _capi
from .common import STREAM32_VARIANT, STREAM64_VARIANT, STREAM_VARIANT, STREAM_VARIANTS, _TLS
from .decoder import ConvChainOp


class TunedPlan(object):
    """what DirEngine inherits: `forward`, `tuned_batches`, `_tuned_order`, `pending_tuning` and `device` are the engine's"""

    # kernel variants a layer can be forced to (include/dir_hip.h: DIR_CONV_VARIANT); 0 = the library's heuristic.  (Code 19, the
    # 64x128 tile on the 3-buffer ring, is not offered: see conv.hip, DIR_RING_64x128.)
    # All of them -- including the streaming 1x1 kernel (STREAM_VARIANT, stream.hip), which feeds the MFMA the same k-slots in the
    # same order as the tiled kernels -- accumulate identically: outputs are bit-identical whichever is chosen
    # (tools/check_stream_layers.py, tests/test_gpu_dir.py::test_autotuned_engine_is_bit_identical).
    # (STREAMP_VARIANT = 24, the pipelined streaming kernel of round 5, is built, bit-identical and tested but NOT offered: measured slower than 21 / 22 on
    #  every layer it could serve -- one producer wave cannot issue 16 KB of LDS-DMA per 0.25 us of MFMAs; tools/bench_stream.py, docs/rounds/DESIGN_rounds_1_to_5.md 11)
    CONV_VARIANTS = (0, 1, 2, 3, 4, 17, 18, 20, 8, 9, 10, 11, 12, 13, 14, 15, STREAM_VARIANT, STREAM64_VARIANT, STREAM32_VARIANT, 25, 26, 27, 28)

    def _profiled_forwards(self, img, n):
        """n eager forwards with every library call timed; returns the records of the conv family (those that carry an `op`).
        A caller's own _capi.PROFILE list is left as it was and is set again afterwards."""
        saved_profile, _capi.PROFILE = _capi.PROFILE, []
        try:
            for _ in range(n):
                self.forward(img)
            torch.cuda.synchronize()
            return [r for r in _capi.PROFILE if r.get('op') is not None]
        finally:
            _capi.PROFILE = saved_profile

    # margin by which an 8-wave one-workgroup-per-CU variant (pipe / patch) must beat the best 4-wave variant in isolation (A/B aid)
    PIPE_MARGIN = float(os.environ.get('DIR_TUNE_PIPE_MARGIN', '0.03'))
    TUNE_EXCLUDE = tuple(int(v) for v in os.environ.get('DIR_TUNE_EXCLUDE', '').split(',') if v)   # variants autotune skips (A/B aid)
    STREAM_MARGIN = float(os.environ.get('DIR_TUNE_STREAM_MARGIN', '0.03'))     # same for the streaming 1x1 kernel (negative: preferred even when slower alone)

    def autotune(self, img, reps=2):
        """Pick the convolution kernel variant per layer for this batch size by timing every candidate inside real
        forwards (HIP events around each conv launch, one stream, realistic cache state).  All variants accumulate in
        the same order, so the outputs are bit-identical whatever is chosen; a variant that does not apply to a layer falls
        back to the heuristic inside the library.  ~14 x (reps+1) eager forwards, once per (engine, batch size)."""
        B = img.shape[0]
        best, covers = {}, {}
        try:
            for v in self.CONV_VARIANTS:
                if v in self.TUNE_EXCLUDE:
                    continue
                _TLS.variant = v
                self._profiled_forwards(img, 1)                    # warm-up (allocator, instruction cache)
                acc = {}
                for rec in self._profiled_forwards(img, reps):
                    acc.setdefault(rec['op'], []).append(rec['e0'].elapsed_time(rec['e1']))
                    covers[rec['op']] = rec.get('covers', ())
                for op, ts in acc.items():
                    t = min(ts)
                    margin = self.PIPE_MARGIN if v in (8, 9, 10, 11, 12, 13, 14, 15) else self.STREAM_MARGIN if v in STREAM_VARIANTS else 0.03
                    if op not in best or t < best[op][0] * (1.0 - margin):  # a challenger must win by 3 % (timing noise)
                        best[op] = (t, v)
        finally:
            _TLS.variant = None
        for op, (t, v) in best.items():
            op.variant[B] = v
        self.tuned_batches.add(B)
        # first-call order of one forward: stable for a given engine.  One row per LAYER: a chained launch (ConvChainOp) is followed by the layers it
        # covers, whose variant is carried (it is what they run with when the chain is off)
        self._tuned_order[B] = self._layer_ops(dict(op=op, covers=covers.get(op, ())) for op in best)
        for op in self._tuned_order[B]:
            op.variant.setdefault(B, 0)
        return {op: op.variant[B] for op in self._tuned_order[B]}

    @staticmethod
    def _layer_ops(recs):
        """the conv-family layers behind profile records, in first-call order: a record's op, then the ops its launch covers"""
        ops = []
        for rec in recs:
            for op in (rec['op'],) + tuple(rec.get('covers', ())):
                if op not in ops:
                    ops.append(op)
        return ops

    def autotune_energy(self, img, seconds=None, slack=2.6, idle_w=None, log=None, max_calls=None, min_saving=0.0, near=1.12):
        """The per-layer kernel choice for THROUGHPUT with several forwards in flight.  Four bs-64 forwards in flight run the socket at its
        power cap (docs/rounds/DESIGN_rounds_1_to_5.md 9: 1.3-1.4 kW of 1.4 kW, 2.9 J per forward), so what raises images/s is the variant that costs the fewest joules
        above idle, not the one that finishes first alone: typically a larger tile on fewer CUs (less L2 -> LDS and LDS -> register traffic
        per MFMA), the idle CUs being filled by the other forwards.  Every convolution call of one forward is captured and replayed back to
        back on its real tensors, per variant, for `seconds`, and its energy is read from the socket's energy accumulator (amdsmi: exact joules
        over the window; default 0.2 s) or, where that is not available, from rocm-smi's averaged power sampled over the last 40 % of a longer
        window (default 0.8 s: the reading lags by about a second); the choice minimises joules above idle per launch among the variants within
        `slack` x the fastest.  ~50 calls x ~10 variants x seconds: 2 minutes with the counter, 5-8 without -- run it
        once per (GPU model, batch size) and keep export_tuning()'s table (dir_amd/tuning/, load_tuning_table).  Results stay bit-identical
        (same argument as autotune).  One forward alone gets ~15 % slower with this table: latency-bound callers keep autotune().
        min_saving (round 6): a variant slower than `near` x the fastest is taken only if it saves at least this fraction of the joules of the best
        variant that IS within `near` x the fastest.  With 0 (rounds 3-5) the table held a dozen launches that were 1.4 - 2.5x slower one at a time for
        1 - 5 % fewer joules -- inside the 0.2 s windows' noise -- which cost 0.17 ms of one-forward latency and a tenth of the per-launch roofline
        fraction for nothing measurable at four in flight (profiles/r06_energy_rule_ab.txt)."""
        import time as _time
        from .. import power
        B = img.shape[0]
        if B not in self._tuned_order:
            self.autotune(img)                                         # the time-tuned choice first: op order, and the fallback for every op not replayed here
        counter = power.energy_joules() is not None
        if not counter and power.smi_sample() is None:
            raise RuntimeError('autotune_energy: neither the amdsmi energy counter nor rocm-smi gives a reading on this machine')
        if seconds is None:
            seconds = 0.2 if counter else 0.8
        torch.cuda.synchronize(self.device)
        if idle_w is None:
            idle_w = power.IDLE_W       # (the reading is a moving average with a time constant near a second: an "idle" sample taken here would still carry load)
        rows = []
        try:
            _TLS.capture = []
            self.forward(img)
            torch.cuda.synchronize(self.device)
            calls, _TLS.capture = _TLS.capture, None
            seen = set()
            for op, args, kw in (calls if max_calls is None else calls[:max_calls]):      # (max_calls: tests rate the first few calls only)
                if id(op) in seen:                                     # an op called twice per forward keeps one choice: the first call's
                    continue
                seen.add(id(op))
                times = {}
                for v in self.CONV_VARIANTS:
                    if v in self.TUNE_EXCLUDE:
                        continue
                    _TLS.variant = v
                    for _ in range(3):
                        op(*args, **kw)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        op(*args, **kw)
                    e1.record()
                    torch.cuda.synchronize(self.device)
                    times[v] = e0.elapsed_time(e1) / 10 * 1e3
                tb = min(times.values())
                row = {}
                for v, us in times.items():
                    if us > slack * tb:
                        continue
                    _TLS.variant = v
                    burst = max(10, min(100, int(0.02 / (us * 1e-6))))                  # ~20 ms of launches between host synchronisations
                    if counter:
                        for _ in range(burst):                                          # the loop is already running when the counter is read
                            op(*args, **kw)
                        torch.cuda.synchronize(self.device)
                        e0 = power.energy_joules()
                    else:
                        smp = power.Sampler(skip=0.6 * seconds, period=0.03).start()    # the first 60 % still carries the previous variant's level
                    t0, n = _time.perf_counter(), 0
                    while _time.perf_counter() - t0 < seconds:
                        for _ in range(burst):
                            op(*args, **kw)
                        torch.cuda.synchronize(self.device)
                        n += burst
                    dt = _time.perf_counter() - t0
                    if counter:
                        e1 = power.energy_joules()
                        w = (e1[0] - e0[0]) / dt if e0 and e1 else float('nan')
                    else:
                        w = power.median(smp.stop(), 'w')
                    if w == w:                                         # (NaN: no reading in the window -- variant not rated)
                        row[v] = (dt / n * 1e6, w)
                _TLS.variant = None
                if not row:
                    continue
                joules = lambda v: row[v][0] * max(row[v][1] - idle_w, 1.0)  # noqa: E731
                fastest = min(row, key=lambda v: row[v][0])
                base = min((v for v in row if row[v][0] <= near * row[fastest][0]), key=joules)
                best = min(row, key=joules)
                if joules(best) > (1.0 - min_saving) * joules(base):
                    best = base
                op.variant[B] = best
                rows.append(dict(cout=op.cout, cin=getattr(op, 'cin', 0), kh=getattr(op, 'kh', 1), stride=getattr(op, 'stride', 1), chosen=best,
                                 us=round(row[best][0], 1), w=round(row[best][1]), fastest=fastest, fastest_us=round(row[fastest][0], 1),
                                 fastest_w=round(row[fastest][1])))
                if log is not None:
                    log(rows[-1])
                for c in ((op.c1,) if isinstance(op, ConvChainOp) else ()):       # a layer covered by a chained launch is not rated (no row in `layers`:
                    c.variant.setdefault(B, 0)                                    # those are measurements); its variant is carried in the table
        finally:
            _TLS.capture, _TLS.variant = None, None
        return {'idle_w': idle_w, 'layers': rows, 'instrument': 'amdsmi energy accumulator, %.2f s windows' % seconds if counter else 'rocm-smi power, last 40 %% of %.2f s windows' % seconds}

    TUNING_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tuning')      # dir_amd/tuning

    def load_tuning_table(self, img, name):
        """Apply dir_amd/tuning/<name>.json (written by tools/energy_tune.py from export_tuning) if it was made for this batch size and an
        identically built engine; returns the table's meta dict, or None when there is no such table / it does not match (the caller then
        keeps whatever autotune chose)."""
        path = os.path.join(self.TUNING_DIR, name + '.json')
        if not os.path.exists(path):
            return None
        with open(path) as f:
            t = json.load(f)
        if t.get('batch') != img.shape[0] or any(int(r[5]) not in self.CONV_VARIANTS for r in t['table']):
            return None
        try:
            self.import_tuning(img, t['table'])
        except ValueError:
            return None
        return t.get('meta', {})

    def export_tuning(self, B):
        """the variants autotune chose for batch size B, in the order the conv layers run (JSON-serialisable)"""
        return [[op.cout, op.cin, op.kh, op.kw, op.stride, op.variant.get(B, 0)] for op in self._tuned_order[B]]

    def import_tuning(self, img, table):
        """apply a table produced by export_tuning on an identically built engine (same layer order, checked by shape)"""
        B = img.shape[0]
        ops = self._layer_ops(self._profiled_forwards(img, 1))      # (a chained launch stands for every layer it covers)
        if len(ops) != len(table) or any([op.cout, op.cin, op.kh, op.kw, op.stride] != row[:5] for op, row in zip(ops, table)):
            raise ValueError('tuning table does not match this engine')
        for op, row in zip(ops, table):
            op.variant[B] = int(row[5])
        self.tuned_batches.add(B)
        self._tuned_order[B] = ops

    def export_all_tuning(self):
        return {B: self.export_tuning(B) for B in self._tuned_order}

    def tune_for(self, img):
        """Make sure batch size img.shape[0] has a kernel choice: a table handed over from the previous engine, else the variants of
        the nearest batch size already tuned (the ragged last batch of an evaluation loader must not cost 45 forwards), else a
        timed autotune."""
        B = img.shape[0]
        if B in self.tuned_batches:
            return
        if self.pending_tuning and B in self.pending_tuning:
            try:
                self.import_tuning(img, self.pending_tuning[B])
                return
            except ValueError:
                pass
        if self._tuned_order:
            self.copy_tuning(min(self._tuned_order, key=lambda b: abs(b - B)), B)
        else:
            self.autotune(img)

    def copy_tuning(self, B_from, B_to):
        """reuse the variants tuned for batch size B_from at batch size B_to (e.g. the ragged last batch of an evaluation loader:
        the choice is bit-identical by construction, so only speed is at stake)"""
        for op in self._tuned_order.get(B_from, []):
            op.variant[B_to] = op.variant.get(B_from, 0)
        self._tuned_order[B_to] = self._tuned_order[B_from]
        self.tuned_batches.add(B_to)
