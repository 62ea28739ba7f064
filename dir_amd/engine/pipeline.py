"""Several forwards in flight: one captured HIP graph of DirEngine.forward per slot."""
import torch


class ForwardPipeline(object):
    """Several forwards in flight: one captured HIP graph of `DirEngine.forward` per slot, each with its own stream, input
    tensor and activation / output buffers (the weights are the engine's, shared).  Images are independent
    (models/dir.py:513-540 has no cross-sample op in eval mode), so two batches can overlap freely: the low-occupancy token
    kernels (64-336 workgroups) and every kernel's ramp / drain of one forward run under the convolutions of the other.
    Measured at B = 64, bf16: 2.93 ms per forward with one in flight, 2.44 ms with two (three: slower -- cache and LDS
    contention), `tools/two_stream_test.py`.

        pipe = ForwardPipeline(eng, [img_a, img_b])      # static input tensor per slot
        pipe.refill(0, batch0); pipe.launch(0); pipe.refill(1, batch1); pipe.launch(1)
        outs = pipe.wait(0)                               # host wait; valid until slot 0 is launched again

    Results are bit-identical to `eng.forward(img)`: the same kernels on the same inputs, only scheduled side by side."""

    def __init__(self, eng, imgs, want_proj_feat=True, streams=None):
        """streams: optional list of torch streams to run the slots on (one per slot).  HIP multiplexes streams onto a handful of
        hardware queues (GPU_MAX_HW_QUEUES, default 4 including the null stream's: set it to 8 before the runtime starts for four
        slots, as bench.py does); two slots whose streams share a queue do not overlap at all, so a second pipeline on the same engine
        should re-use the first one's streams (bench.py's proj_feat-less variant does)."""
        assert len(imgs) >= 1 and (streams is None or len(streams) == len(imgs))
        self.eng, self.imgs = eng, list(imgs)
        self.streams, self.graphs, self.outs, self.done = [], [], [], []
        cur = torch.cuda.current_stream()
        for i, img in enumerate(self.imgs):
            s = streams[i] if streams is not None else torch.cuda.Stream(device=eng.device)
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                eng.forward(img, want_proj_feat)          # eager once on this stream: allocator warm-up before the capture
                s.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    o = eng.forward(img, want_proj_feat)
            self.streams.append(s); self.graphs.append(g); self.outs.append(o)
            self.done.append(torch.cuda.Event())
        torch.cuda.synchronize(eng.device)

    def __len__(self):
        return len(self.graphs)

    def refill(self, slot, batch):
        """Copies `batch` into the slot's input ON THE SLOT'S STREAM (ordered before its next launch by stream order alone).
        `batch` must be complete from the host's point of view (pinned host memory, or device memory produced before a host
        synchronise): every hand-over of the pipeline is stream order or a host wait, no cross-stream event edges."""
        with torch.cuda.stream(self.streams[slot]):
            self.imgs[slot].copy_(batch, non_blocking=True)

    def launch(self, slot):
        """Replays slot's forward on its stream (after whatever `refill` queued there)."""
        s = self.streams[slot]
        with torch.cuda.stream(s):
            self.graphs[slot].replay()
            self.done[slot].record(s)

    def wait(self, slot):
        """Host wait for slot's forward; returns its outs_list (valid until the slot is launched again)."""
        self.done[slot].synchronize()
        return self.outs[slot]
