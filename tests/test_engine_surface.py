"""dir_amd.engine is a package; this pins the surface the single module engine.py had before it was split: every name it bound at module
level is still an attribute of dir_amd.engine, every class and function is the SAME object as in the module that now holds it (a duplicate
would let `E.BackboneOp.l3_chain = False` flip a switch nothing reads), _TLS is one object, and the class-level switches and the tuning
interface are where tests and tools reach for them.  Host only."""
import importlib
import inspect
import os

from dir_amd import engine as E

# every name engine.py bound at module level (ast over its last single-file version), without the imported modules C, math, json, os, threading, torch
NAMES = ('_capi', 'CONV_PRE_RELU', 'CONV_RELU', 'DT_BF16', 'DT_F16', 'DT_F16X1', 'DT_F16X1P', 'DT_F16X3', 'DT_F16X3P', 'DT_F32', 'ConvDesc',
         'pack_as_weights', 'pack_l3_stream', 'pack_stream_weights', 'pack_tail_stream', 'F32', 'IMAGENET_MEAN', 'IMAGENET_STD', '_ThreadState',
         '_TLS', '_variant_for', '_packing_arith', '_ann', 'HALF', '_dt', '_tok_wdt', 'bn_fold', 'STREAM_VARIANT', 'STREAM64_VARIANT',
         'STREAM32_VARIANT', 'STREAMP_VARIANT', 'STREAM_VARIANTS', 'AS_VARIANTS', 'ConvOp', 'DualConvOp', 'pack_token_mlp', 'pack_pgcn', 'pack_ste',
         '_pad_rows', 'pack_mano', 'BneckChainOp', 'BneckTailOp', 'BneckBlockOp', 'stem_conv_op', 'BackboneOp', 'backbone_standalone', '_padc',
         '_pad_conv_bn', 'HRNetOp', 'hrnet_standalone', 'ResidualOp', 'ConvChainOp', 'StageOp', 'run_mano_pair', 'DirEngine', 'ForwardPipeline')

SUBMODULES = ('common', 'conv', 'backbone', 'hrnet', 'decoder', 'stage', 'autotune', 'plan', 'pipeline')


def _submodules():
    return [importlib.import_module('dir_amd.engine.' + m) for m in SUBMODULES]


def test_every_name_of_the_old_module_is_exported():
    assert len(NAMES) == len(set(NAMES)) == 56
    missing = [n for n in NAMES if not hasattr(E, n)]
    assert not missing, missing


def test_classes_and_functions_are_the_objects_of_their_modules():
    for n in NAMES:
        obj = getattr(E, n)
        if not (inspect.isclass(obj) or inspect.isfunction(obj)):
            continue
        home = importlib.import_module(obj.__module__)
        assert getattr(home, n) is obj, n
        for m in _submodules():                        # and wherever else a submodule has the name, it is that object too
            if hasattr(m, n):
                assert getattr(m, n) is obj, (m.__name__, n)


def test_tls_is_one_object():
    holders = [m for m in _submodules() if hasattr(m, '_TLS')]
    assert len(holders) >= 5                           # conv, backbone, decoder, autotune, plan read it; common makes it
    for m in holders:
        assert m._TLS is E._TLS, m.__name__
    assert isinstance(E._TLS, E._ThreadState)


def test_switches_live_on_their_classes():
    for cls, attrs in ((E.ConvOp, ('PRESPLIT', 'OUT_SPLIT')),
                       (E.BackboneOp, ('fused_stem', 'bneck_chain', 'bneck_tail', 'l3_chain', 'decimate_c1')),
                       (E.ResidualOp, ('res_chain',)),
                       (E.ConvChainOp, ('head_chain',)),
                       (E.DirEngine, ('factorised_fusion', 'PIPE_MARGIN', 'TUNE_EXCLUDE', 'STREAM_MARGIN'))):
        for a in attrs:
            assert hasattr(cls, a), (cls.__name__, a)


def test_direngine_keeps_its_interface():
    for a in ('autotune', 'autotune_energy', 'load_tuning_table', 'export_tuning', 'import_tuning', 'export_all_tuning', 'tune_for', 'copy_tuning',
              'calibrate', 'forward', 'stage', 'init_regressor', 'mano_outputs', 'upsample_into', 'CONV_VARIANTS', 'PIPE_MARGIN', 'TUNE_EXCLUDE',
              'STREAM_MARGIN'):
        assert hasattr(E.DirEngine, a), a


def test_tuning_dir_is_dir_amd_tuning():
    assert os.path.isfile(os.path.join(E.DirEngine.TUNING_DIR, 'gfx950_bf16_b64_throughput.json'))
    assert os.path.basename(os.path.dirname(E.DirEngine.TUNING_DIR)) == 'dir_amd'


def test_engine_is_a_package():
    here = os.path.dirname(os.path.abspath(E.__file__))
    assert os.path.basename(E.__file__) == '__init__.py' and os.path.basename(here) == 'engine'
    assert not os.path.exists(os.path.join(os.path.dirname(here), 'engine.py'))
