def checkpoint_weights(ck, ema=False, path='the checkpoint'):
    """the state dict a command-line tool loads from what torch.load gave it: ck['net'] (train.py's checkpoints) or ck itself (a bare
    state dict); ema: ck['ema'], the averaged weights that dir_amd.apps.train --ema_decay writes next to 'net'"""
    if ema:
        if not isinstance(ck, dict) or 'ema' not in ck:
            raise KeyError("--ema: %s holds no averaged weights (no 'ema' key: it was not written by dir_amd.apps.train --ema_decay)" % path)
        return ck['ema']
    return ck['net'] if isinstance(ck, dict) and 'net' in ck else ck
