"""Host-side mirror of the reference's train.py on libdir_hip.so: one command trains a DIR model.

    python -m dir_amd.apps.train --data_path ROOT --output_root OUT --init CKPT [--total_epoch 50] [--bs 64] [--lr 5e-4] ...

  ValMetrics      InterHandDataset.evaluate (dataset/interhand.py:262-315) + the sums of Trainer.test_model (train.py:160-181): ONE
                  dir_val_metrics_forward call per batch covers every stage; the sums stay on the GPU until result()
  validate        Trainer.test_model (train.py:156-202): eval-mode forwards of the 16-bit engine over a split in file order, the
                  reference's MPJPE_i / MPVPE_i lines, -> dict ('error' = the number that selects best.pth)
  fit             train() (train.py:58-91) around dir_amd.train.step (GraphedTrainStep | train_step | the module's own four lines):
                  the loop, the log line, the pictures, schedule.step(), latest.pth / best.pth
  main            the command line; Trainer._make_model / _make_batch_loader (train.py:204-243)

The MANO buffers and faces come from the --init checkpoint, as everywhere in this project.  Not copied from train.py: img_size is 256
(train.py:207 passes cfg.root_joint), the source tree is not copied into the output folder.  Not built: more than one rank (the step
functions average gradients when torch.distributed is initialised, but this driver shards nothing and every rank would log and save).
"""
import contextlib
import logging
import math
import os
import sys
import time

import numpy as np
import torch

from .. import _capi

SIDES = ('left', 'right')
DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
MAX_STAGES = 8              # DIR_VAL_MAX_STAGES


class ValMetrics(object):
    """m = ValMetrics(n_stages); m.update(outs_list, targets) per batch (one library call, no host synchronisation); m.result() reads
    the sums (the only host read).  outs_list[s]: 'pd_joint_xyz_*' [B,21,3], 'pd_mesh_xyz_*' [B,778,3]; targets: 'joint_3d_*', 'mesh_3d_*'."""

    def __init__(self, n_stages=3):
        if not 1 <= int(n_stages) <= MAX_STAGES:
            raise ValueError('ValMetrics: n_stages must be in 1..%d, got %r' % (MAX_STAGES, n_stages))
        self.n_stages = int(n_stages)
        self.acc, self.batches, self.sample_sums = None, None, None

    def reset(self):
        if self.acc is not None:
            self.acc.zero_()
            self.batches.zero_()

    def update(self, outs_list, targets):
        if len(outs_list) < self.n_stages:
            raise ValueError('ValMetrics.update: %d stage dicts, %d expected' % (len(outs_list), self.n_stages))
        pd = [[outs_list[s][k + side] for side in SIDES] for s in range(self.n_stages) for k in ('pd_joint_xyz_', 'pd_mesh_xyz_')]
        gt = [[targets[k + side] for side in SIDES] for k in ('joint_3d_', 'mesh_3d_')]
        _capi.require_cuda(*[t for pair in pd + gt for t in pair])
        pd = [[_capi.f32c(t) for t in pair] for pair in pd]
        gt = [[_capi.f32c(t) for t in pair] for pair in gt]
        B, dev = gt[0][0].shape[0], gt[0][0].device
        for i, pair in enumerate(pd + gt):
            for t in pair:
                shp = (B, 21 if i % 2 == 0 else 778, 3)
                if tuple(t.shape) != shp or t.device != dev:
                    raise _capi.DirHipError('ValMetrics.update: tensor of shape %s on %s where %s on %s is expected' % (tuple(t.shape), t.device, shp, dev))
        if self.acc is None or self.acc.device != dev:
            self.acc = torch.zeros(self.n_stages, 4, dtype=torch.float64, device=dev)
            self.batches = torch.zeros(1, dtype=torch.int64, device=dev)
        if self.sample_sums is None or self.sample_sums.shape[1] != B or self.sample_sums.device != dev:
            self.sample_sums = torch.zeros(self.n_stages, B, 4, dtype=torch.float64, device=dev)
        d = _capi.ValMetricsDesc()
        for s in range(self.n_stages):
            for h in range(2):
                d.joints_pd[s][h], d.verts_pd[s][h] = pd[2 * s][h].data_ptr(), pd[2 * s + 1][h].data_ptr()
        for h in range(2):
            d.joints_gt[h], d.verts_gt[h] = gt[0][h].data_ptr(), gt[1][h].data_ptr()
        d.sample_sums, d.acc, d.batches = self.sample_sums.data_ptr(), self.acc.data_ptr(), self.batches.data_ptr()
        with torch.cuda.device(dev):
            _capi.check(_capi.lib().dir_val_metrics_forward(d, self.n_stages, B, _capi.stream_ptr()), 'dir_val_metrics_forward')

    def result(self):
        """train.py:177-202: {'MPJPE_<i>' / 'MPVPE_<i>': {'left', 'right', 'all'}, 'batches': n, 'error': the last stage's MPJPE 'all'}"""
        if self.acc is None:
            n, acc = 0, np.zeros((self.n_stages, 4))
        else:
            n, acc = int(self.batches.cpu()[0]), self.acc.cpu().numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = acc / np.float64(n)                        # no batch: nan, as the reference's 0 / 0
        res = {'batches': n}
        for s in range(self.n_stages):
            for name, o in (('MPJPE_%d' % s, 0), ('MPVPE_%d' % s, 2)):
                l, r = float(mean[s, o]), float(mean[s, o + 1])
                res[name] = {'left': l, 'right': r, 'all': (l + r) / 2}
        res['error'] = res['MPJPE_%d' % (self.n_stages - 1)]['all']
        return res


def _n_stages(model):
    return 3 + int(getattr(model, 'extra_stages', 0))


def report_lines(res, n_stages):
    """-> (the lines train.py:183-188 prints, the lines train.py:190-199 logs)"""
    printed, logged = [], []
    for s in range(n_stages):
        for name in ('MPJPE_%d' % s, 'MPVPE_%d' % s):
            m = res[name]
            printed += ['%s:' % name, '    left: {} mm, right: {} mm'.format(m['left'], m['right']), '    all: {} mm'.format(m['all'])]
            logged.append('{}: left {} mm, right {} mm, AVG {} mm'.format(name, m['left'], m['right'], m['all']))
    return printed, logged


def validate(model, batches, logger=None, dtype=None, quiet=False, penetration=False, aligned=False):
    """Trainer.test_model (train.py:156-202).  model: a dir_amd.models.dir.DIR on the GPU; batches: an iterable of (inputs, targets,
    meta_info) -- TrainBatches(data_path, gt_layers, split, batch_size, augment=False, shuffle=False); one with `seed` and `rng` is re-seeded
    first, so that every validation sees the same noise.  dtype: the feature-map type of the eval-mode engine (torch.float16 |
    bfloat16 | float32; None = model.compute_dtype as it is).  The packed engine is dropped first (model.refresh()): training writes BatchNorm
    running statistics through raw pointers, which no version counter sees.
    penetration: also measure how far the last stage's two hands pass through each other (utils/penetration.py, wrists as the face table
    has them, no volume): adds 'penetration_depth_mm' (mean over the samples) and 'penetration_rate' (share of samples with a penetrating
    vertex) to the result and one line to the report; 'error', which selects best.pth, is not touched.
    aligned: also the last stage's errors after a per-hand similarity alignment (utils/alignment.py: joints on joints, vertices on vertices,
    with scale, proper rotations only), from the same 'pd_joint_xyz_*' / 'pd_mesh_xyz_*' and targets ValMetrics reads: adds 'PA_MPJPE_<last>' and
    'PA_MPVPE_<last>' as {'left', 'right', 'all'} (mm; a hand whose joint or mesh alignment does not exist is left out of both, as AlignedMetrics
    does) and one line to the report; 'error' is not touched."""
    _capi.require_cuda(*list(model.parameters()))
    if dtype is not None:
        model.compute_dtype = dtype
    n_stages = _n_stages(model)
    metrics = ValMetrics(n_stages)
    pen = None
    if penetration:
        from ..utils import penetration as PN
        from ..utils.vis_utils import two_hand_faces
        dev = next(model.parameters()).device
        pen = PN.PenetrationMetrics(PN.hand_faces(two_hand_faces(model.init_regressor.mano_layer_right.th_faces.cpu().numpy()), device=dev)[:2],
                                    stage_num=n_stages, volume_pitch=None)
    pa_sums, pa_points = [], None
    if aligned:
        from ..utils.alignment import procrustes_align
    if hasattr(batches, 'rng') and hasattr(batches, 'seed'):
        batches.rng = np.random.default_rng(batches.seed)
    model.eval()
    model.refresh()
    try:
        with torch.no_grad():
            for inputs, targets, meta_info in batches:
                outs_list, _ = model(inputs, targets, meta_info)
                metrics.update(outs_list, targets)
                if pen is not None:
                    pen.update(outs_list)
                if aligned:
                    last = outs_list[n_stages - 1]
                    # per-sample sums in float64 (NaN: no alignment exists), read once after the loop
                    pa_sums.append(torch.stack([procrustes_align(last[k + side], targets[g + side])['err'].double().sum(1)
                                                for k, g in (('pd_joint_xyz_', 'joint_3d_'), ('pd_mesh_xyz_', 'mesh_3d_')) for side in SIDES], 1))
                    pa_points = [last[k + side].shape[1] for k in ('pd_joint_xyz_', 'pd_mesh_xyz_') for side in SIDES]
    finally:
        model.train()                                     # train.py:201
    res = metrics.result()
    printed, logged = report_lines(res, n_stages)
    if pen is not None and pen.batches:
        ps = pen.summarize()
        res['penetration_depth_mm'], res['penetration_rate'] = ps['depth_mean_mm'], ps['rate']
        line = 'penetration_{}: depth {} mm, rate {}'.format(n_stages - 1, ps['depth_mean_mm'], ps['rate'])
        printed.append(line)
        logged.append(line)
    if pa_sums:
        sums = torch.cat(pa_sums, 0).cpu().numpy()                          # [n, (joint left, joint right, mesh left, mesh right)]
        for h in range(2):                                                  # a hand without a joint OR a mesh alignment is left out of both
            none = np.isnan(sums[:, h]) | np.isnan(sums[:, 2 + h])
            sums[none, h], sums[none, 2 + h] = np.nan, np.nan
        mean = np.array([np.nanmean(sums[:, c]) if np.isfinite(sums[:, c]).any() else np.nan for c in range(4)]) / pa_points * 1000
        for name, o in (('PA_MPJPE_%d' % (n_stages - 1), 0), ('PA_MPVPE_%d' % (n_stages - 1), 2)):
            l, r = float(mean[o]), float(mean[o + 1])
            res[name] = {'left': l, 'right': r, 'all': (l + r) / 2}
        line = ', '.join('{}: left {} mm, right {} mm, AVG {} mm'.format(k, res[k]['left'], res[k]['right'], res[k]['all'])
                         for k in ('PA_MPJPE_%d' % (n_stages - 1), 'PA_MPVPE_%d' % (n_stages - 1)))
        printed.append(line)
        logged.append(line)
    if not quiet:
        print('\n'.join(printed))
    if logger is not None:
        for l in logged:
            logger.info(l)
    return res


# ---------------------------------------------------------------------------------------------------------------------------- the driver
def setup_logger(output_root, name='DIR'):
    """train.py:105-125 without the colours: <output_root>/log/train_<name>.log and stdout"""
    os.makedirs(os.path.join(output_root, 'log'), exist_ok=True)
    path = os.path.join(output_root, 'log', 'train_%s.log' % name)
    logger = logging.getLogger('Training.%s.%d' % (os.path.abspath(path), time.monotonic_ns()))
    logger.setLevel(logging.DEBUG)
    logger.propagate = False
    fmt = logging.Formatter('[%(asctime)s] Training %(levelname)s: %(message)s', datefmt='%m/%d %H:%M:%S')
    for h in (logging.StreamHandler(sys.stdout), logging.FileHandler(path, mode='a')):
        h.setFormatter(fmt)
        logger.addHandler(h)
    logger.info('Start training: %s' % ('train_' + name))
    return logger


def close_logger(logger):
    for h in list(logger.handlers):
        h.flush()
        if isinstance(h, logging.FileHandler):
            h.close()
        logger.removeHandler(h)


def stage_dicts(outs):
    """the step's own outputs (dir_amd.train.net.forward) as overlay_predictions reads a stage: + 'pd_proj_*' = the last three MANO
    parameters (models/dir.py's scale and 2-D translation); views, nothing is copied"""
    res = []
    for o in outs[:-1]:
        d = {k: o[k] for k in o if k.startswith(('pd_joint_uv_', 'pd_mesh_xyz_', 'pd_joint_xyz_'))}
        for s in SIDES:
            d['pd_proj_' + s] = o['pd_mano_para_' + s][:, 61:]
        res.append(d)
    return res


def draw(outs, inputs, renderer, vis_dir, iteration, batch_size, samples=(0, 1, 2, 3)):
    """train.py:17-55's pictures from the training step's own outputs: for the first four images of the batch and every stage, the predicted
    meshes over the frame (overlay_predictions) with the predicted 2-D joints on top (draw_joints).  <vis>/<id>_pd_<stage>.png, RGB."""
    from PIL import Image
    from ..utils import vis_utils as V
    idx = [i for i in samples if i < inputs['img_rgb'].shape[0]]
    frames = inputs['img_rgb'][idx].round().clamp(0, 255).to(torch.uint8).contiguous()
    os.makedirs(vis_dir, exist_ok=True)
    written = []
    for s, d in enumerate(stage_dicts(outs)):
        sub = {k: v[idx].contiguous() for k, v in d.items()}
        over = V.overlay_predictions(sub, frames, renderer, v_color=renderer.rgb_coor)       # the frames are RGB here
        over = V.draw_joints(over, sub['pd_joint_uv_left'], sub['pd_joint_uv_right']).cpu().numpy()
        for j, i in enumerate(idx):
            path = os.path.join(vis_dir, '%d_pd_%d.png' % (iteration * batch_size + i, s))
            Image.fromarray(over[j]).save(path, format='PNG')
            written.append(path)
    return written


def log_line(epoch, total_epoch, iteration, n_iter, lr, loss):
    """train.py:72-75; `loss`: {key: python float}"""
    return ''.join(['[Epoch %d/%d]' % (epoch, total_epoch), '[Batch %d/%d]' % (iteration, n_iter), '[lr %f]' % lr] +
                   ['[%s: %.4f]' % ('loss_' + k, v) for k, v in loss.items()])


def epoch_rng(seed, epoch):
    """the generator of epoch `epoch`'s permutation, augmentation draws and noise seeds: a function of (seed, epoch) only, so a resumed run
    sees the batches the uninterrupted run would have seen"""
    return np.random.default_rng([int(seed), int(epoch)])


class NonFiniteLoss(RuntimeError):
    pass


def check_finite(total, epoch, iteration):
    """a NaN / inf total loss on a printing iteration ends the run instead of training on"""
    if not math.isfinite(total):
        raise NonFiniteLoss('the total loss is %r at epoch %d, iteration %d: stopping (see the log line above)' % (total, epoch, iteration))


def guard_fields(stats):
    """what a printing iteration's line gains when the guarded step is on; `stats`: FlatAdamW.guard_stats()"""
    return '[grad_norm %.4f][clip %.4f][skipped %d]' % (stats['grad_norm'], stats['clip_coef'], stats['skipped'])


def make_optimizer(model, lr, max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
    """train.py:227 on the module's own parameters (FlatAdamW moves them into one flat buffer; the module keeps seeing them)"""
    from ..optim import FlatAdamW
    from ..train.step import inactive_parameters
    named = dict(model.named_parameters())
    opt = FlatAdamW([{'params': list(named.values()), 'initial_lr': lr}], lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                    ema_decay=ema_decay)
    opt.set_inactive(inactive_parameters(named))
    return opt


def make_schedule(optimizer, lr_scheduler, total_epoch):
    """train.py:229-232"""
    from ..optim import CosineAnnealingLR, MultiStepLR
    if lr_scheduler == 'cosine':
        return CosineAnnealingLR(optimizer, T_max=total_epoch, eta_min=0)
    if lr_scheduler == 'step':
        return MultiStepLR(optimizer, [30], gamma=0.1, last_epoch=-1)
    raise ValueError("lr_scheduler must be 'cosine' or 'step', got %r" % (lr_scheduler,))


def _count_batches(model, steps):
    """nn.BatchNorm's num_batches_tracked, which train_step leaves alone (momentum is not None: the maths never reads it): advanced once per
    epoch by what the module's own training forward adds per step, so checkpoints carry the reference's counts"""
    if steps:
        with torch.no_grad():
            for k, b in model.named_buffers():
                if k.endswith('num_batches_tracked'):
                    b += steps * (2 if ('.global_pos_emb.' in k or '.proj_feat_emb.' in k) else 1)


def fit(model, batches, val_batches=None, output_root='./output', optimizer=None, schedule=None, total_epoch=50, lr=5e-4,
        lr_scheduler='cosine', step='graphed', print_iter=100, draw_iter=100, eval_interval=1, eval_dtype=None, seed=0, max_steps=None,
        continue_train=None, name='DIR', logger=None, on_step=None, eval_penetration=False, eval_aligned=False, max_grad_norm=None,
        skip_nonfinite=False, ema_decay=None):
    """train() of train.py:58-91.  model: a DIR on the GPU, in training mode from here on; batches: TrainBatches of the train split (its
    `rng` is re-seeded per epoch from (seed, epoch)); val_batches: what validate() takes, or None = no validation, no best.pth.
    step: 'graphed' (GraphedTrainStep) | 'eager' (train_step) | 'module' (model(...); sum(loss).backward(); optimizer.step()).
    The driver adds no arithmetic to the step and reads a loss on printing iterations only (iteration % print_iter == 0); a NaN / inf total
    there raises NonFiniteLoss.  on_step(epoch, iteration, global_step): a hook for tests and measurements, called after every step.
    max_grad_norm / skip_nonfinite / ema_decay (none set: nothing below happens): FlatAdamW's guarded step -- clipping by the global norm,
    skipping a step whose gradient is not finite, an average of the weights -- decided on the device; the printing iterations' lines gain
    '[grad_norm ..][clip ..][skipped N]' from one more read there, and NonFiniteLoss is raised when every step since the previous printing
    iteration was skipped.  With ema_decay, validation (and so best.pth) judges the averaged weights, and both checkpoint files carry 'net'
    (raw: what resuming needs), 'ema' and 'guard'.  No accuracy gain from either is shown anywhere in this tree.
    -> {'steps', 'epochs', 'min_error', 'last_val', 'optimizer', 'schedule', 'vis': the pictures written, 'perms': {epoch: the file indices
    in reading order}, 'lrs': {epoch: its learning rate}, 'printed': [(global step, total loss)] of the printing iterations}"""
    from ..optim import load_checkpoint, save_checkpoint
    from ..train import step as TSTEP
    _capi.require_cuda(*list(model.parameters()))
    if step not in ('graphed', 'eager', 'module'):
        raise ValueError("step must be 'graphed', 'eager' or 'module', got %r" % (step,))
    own_logger = logger is None
    logger = setup_logger(output_root, name) if own_logger else logger
    ckpt_dir, vis_dir = os.path.join(output_root, 'checkpoint'), os.path.join(output_root, 'vis')
    for d in (ckpt_dir, vis_dir):
        os.makedirs(d, exist_ok=True)
    try:
        model.train()
        guard_on = max_grad_norm is not None or skip_nonfinite or ema_decay is not None
        if optimizer is None:
            optimizer = make_optimizer(model, lr, max_grad_norm, skip_nonfinite, ema_decay)
        elif guard_on:
            optimizer.configure(max_grad_norm, skip_nonfinite, ema_decay)
        guard_on = bool(getattr(optimizer, 'guarded', False))
        since_print = 0
        schedule = make_schedule(optimizer, lr_scheduler, total_epoch) if schedule is None else schedule
        start_epoch = 0
        if continue_train:
            start_epoch = load_checkpoint(continue_train, model, optimizer, schedule)
            logger.info('Loading the model of epoch-{} from {}...'.format(start_epoch - 1, continue_train))
        named = dict(model.named_parameters())
        buffers = {k: b for k, b in model.named_buffers() if 'num_batches_tracked' not in k}
        faces = (model.init_regressor.mano_layer_left.th_faces, model.init_regressor.mano_layer_right.th_faces)
        graphed = TSTEP.GraphedTrainStep(named, buffers, optimizer, faces) if step == 'graphed' else None
        renderer = None
        state = {'steps': 0, 'epochs': 0, 'min_error': 100, 'last_val': None, 'optimizer': optimizer, 'schedule': schedule, 'vis': [],
                 'perms': {}, 'lrs': {}, 'printed': []}
        stop = False
        for epoch in range(start_epoch, total_epoch):
            batches.rng = epoch_rng(seed, epoch)
            state['lrs'][epoch] = optimizer.param_groups[0]['lr']
            n_iter, done = len(batches), 0
            for iteration, (inputs, targets, meta_info) in enumerate(batches):
                if iteration == 0:
                    state['perms'][epoch] = None if getattr(batches, 'last_perm', None) is None else np.array(batches.last_perm)
                if step == 'graphed':
                    loss = graphed(inputs['img'], targets, meta_info)
                    outs = graphed.outs
                elif step == 'eager':
                    loss = TSTEP.train_step(named, buffers, inputs['img'], targets, meta_info, faces, optimizer)
                    outs = optimizer.last_outs
                else:                                                      # train.py:67-70
                    optimizer.zero_grad()
                    outs_list, loss = model(inputs, targets, meta_info)
                    sum(loss[k] for k in loss).backward()
                    optimizer.step()
                    outs = None
                done += 1
                since_print += 1
                state['steps'] += 1
                if print_iter and iteration % print_iter == 0:            # the loop's only host read
                    vals = torch.stack([v.detach().reshape(()).float() for v in loss.values()]).cpu().tolist()
                    line = log_line(epoch, total_epoch, iteration, n_iter, optimizer.param_groups[0]['lr'], dict(zip(loss, vals)))
                    stats = optimizer.guard_stats() if guard_on else None
                    logger.info(line + (guard_fields(stats) if guard_on else ''))
                    state['printed'].append((state['steps'], sum(vals)))
                    check_finite(sum(vals), epoch, iteration)
                    if guard_on and stats['skipped_in_row'] >= since_print:
                        raise NonFiniteLoss('every one of the %d steps since the previous printing iteration was skipped for a gradient that is '
                                            'not finite (epoch %d, iteration %d; %d skipped in a row): stopping'
                                            % (since_print, epoch, iteration, stats['skipped_in_row']))
                    since_print = 0
                if draw_iter and iteration % draw_iter == 0 and outs is not None:
                    if renderer is None:
                        from ..utils import vis_utils as V
                        renderer = V.mano_two_hands_shaded_renderer(right_faces=faces[1].cpu().numpy(), dense_color=np.zeros((V.NV_HAND, 3)),
                                                                    img_size=inputs['img_rgb'].shape[1], device=inputs['img'].device)
                    state['vis'] += draw(outs, inputs, renderer, vis_dir, iteration, inputs['img'].shape[0])
                if on_step is not None:
                    on_step(epoch, iteration, state['steps'])
                if max_steps is not None and state['steps'] >= max_steps:
                    stop = True
                    break
            _count_batches(model, done if step != 'module' else 0)
            if stop and done < n_iter:
                break                                                      # stopped inside an epoch: nothing is saved for it
            schedule.step()
            save_checkpoint(os.path.join(ckpt_dir, 'latest.pth'), model, optimizer, schedule, epoch)
            logger.info('Save checkpoint to {}'.format(os.path.join(ckpt_dir, 'latest.pth')))
            state['epochs'] += 1
            if val_batches is not None and not epoch % eval_interval:
                # with an average, validation and best.pth judge the averaged weights; the raw ones are back afterwards, bit for bit
                with (optimizer.ema_weights() if getattr(optimizer, 'flat_ema', None) is not None else contextlib.nullcontext()):
                    res = validate(model, val_batches, logger=logger, dtype=eval_dtype, penetration=eval_penetration, aligned=eval_aligned)
                state['last_val'] = res
                if res['error'] < state['min_error']:
                    save_checkpoint(os.path.join(ckpt_dir, 'best.pth'), model, optimizer, schedule, epoch)
                    logger.info('Save checkpoint to {}'.format(os.path.join(ckpt_dir, 'best.pth')))
                    state['min_error'] = res['error']
            if stop:
                break
        return state
    finally:
        if own_logger:
            close_logger(logger)


def init_model(model, state, scope='all'):
    """overwrite the fresh initialisation with the checkpoint's tensors: 'mano' = the MANO buffers only, 'backbone' = those and backbone.*,
    'all' = every tensor (strict)"""
    if scope == 'all':
        model.load_state_dict(state, strict=True)
        return sorted(state)
    if scope not in ('mano', 'backbone'):
        raise ValueError("init_scope must be 'mano', 'backbone' or 'all', got %r" % (scope,))
    own = model.state_dict()
    take = [k for k in own if 'mano_layer' in k or (scope == 'backbone' and k.startswith('backbone.'))]
    missing = [k for k in take if k not in state]
    if missing:
        raise KeyError('--init lacks %d tensors of scope %r, e.g. %s' % (len(missing), scope, missing[0]))
    merged = {k: (state[k] if k in take else v) for k, v in own.items()}
    model.load_state_dict(merged, strict=True)
    return take


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description='train a DIR model on a prepared InterHand2.6M split on MI355X (train.py of the reference)')
    ap.add_argument('--data_path', type=str, default='./data/interhand2.6m/')
    ap.add_argument('--output_root', type=str, default='./output')
    ap.add_argument('--experiment_name', type=str, default='DIR')
    ap.add_argument('--init', type=str, required=True, help='a checkpoint: the MANO buffers and faces come from it')
    ap.add_argument('--init_scope', choices=['mano', 'backbone', 'all'], default='all', help='which of its tensors overwrite the fresh initialisation')
    ap.add_argument('--continue_train', type=str, default=None, help='resume from this latest.pth / best.pth')
    ap.add_argument('--total_epoch', type=int, default=50)
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--lr', type=float, default=5e-4)
    ap.add_argument('--lr_scheduler', choices=['cosine', 'step'], default='cosine')
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eval_split', type=str, default='test')
    ap.add_argument('--eval_interval', type=int, default=1)
    ap.add_argument('--eval_bs', type=int, default=None, help='default: --bs')
    ap.add_argument('--eval_dtype', choices=sorted(DTYPES), default='f16')
    ap.add_argument('--print_iter', type=int, default=100)
    ap.add_argument('--draw_iter', type=int, default=100, help='0 = no pictures')
    ap.add_argument('--dense_color', type=str, default=None, help='the dense colour table: render mask / dense per batch instead of reading them')
    ap.add_argument('--step', choices=['graphed', 'eager', 'module'], default='graphed')
    ap.add_argument('--max_steps', type=int, default=None, help='stop early (tests, smoke runs)')
    ap.add_argument('--backbone', choices=['resnet50', 'hrnet_w48'], default='resnet50')
    ap.add_argument('--extra_stages', type=int, default=0)
    ap.add_argument('--eval_penetration', action='store_true', help="add the last stage's mean inter-hand penetration depth and penetration rate to "
                    'the validation lines (best.pth is still chosen by the joint error)')
    ap.add_argument('--eval_aligned', action='store_true', help="add the last stage's PA-MPJPE and PA-MPVPE (errors after a per-hand similarity "
                    'alignment) to the validation lines (best.pth is still chosen by the unaligned joint error)')
    ap.add_argument('--max_grad_norm', type=float, default=None, help='clip the gradient to this global L2 norm (clip_grad_norm_), on the device')
    ap.add_argument('--skip_nonfinite', action='store_true', help='skip an optimiser step whose gradient holds a NaN or an Inf, on the device; '
                    'the run stops when every step between two printing iterations was skipped')
    ap.add_argument('--ema_decay', type=float, default=None, help="keep an exponential moving average of the weights (e.g. 0.9998): validation and "
                    "best.pth judge it, checkpoints carry it as 'ema' next to 'net'")
    return ap


def main(argv=None):
    """python -m dir_amd.apps.train -> fit()'s dict"""
    from ..models.dir import DIR
    from .dataset import gt_layers_from_checkpoint
    from .trainset import TrainBatches
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise _capi.DirHipError('dir_amd.apps.train runs on the GPU only (no CPU fallback exists)')
    ck = torch.load(opt.init, map_location='cpu', weights_only=False)
    ck = ck['net'] if isinstance(ck, dict) and 'net' in ck else ck
    torch.manual_seed(opt.seed)
    model = DIR(21, 'unused', 0, compute_dtype=DTYPES[opt.eval_dtype], extra_stages=opt.extra_stages, backbone=opt.backbone)
    init_model(model, ck, opt.init_scope)
    model = model.cuda()
    mano = gt_layers_from_checkpoint(ck)
    batches = TrainBatches(opt.data_path, mano, 'train', batch_size=opt.bs, workers=opt.workers, seed=opt.seed, dense_color=opt.dense_color)
    val = None
    if opt.eval_interval > 0:
        val = TrainBatches(opt.data_path, mano, opt.eval_split, batch_size=opt.eval_bs or opt.bs, workers=opt.workers, seed=opt.seed,
                           augment=False, shuffle=False, dense_color=opt.dense_color)
    return fit(model, batches, val, output_root=opt.output_root, total_epoch=opt.total_epoch, lr=opt.lr, lr_scheduler=opt.lr_scheduler,
               step=opt.step, print_iter=opt.print_iter, draw_iter=opt.draw_iter, eval_interval=max(1, opt.eval_interval), seed=opt.seed,
               max_steps=opt.max_steps, continue_train=opt.continue_train, name=opt.experiment_name, eval_penetration=opt.eval_penetration, eval_aligned=opt.eval_aligned,
               max_grad_norm=opt.max_grad_norm, skip_nonfinite=opt.skip_nonfinite, ema_decay=opt.ema_decay)


if __name__ == '__main__':
    main()
