"""The four MANO fitting wrappers of dir_amd.functional share one argument checker (functional._mano_per_hand); the error it raises names the wrapper
that was called.  No GPU: the shape check comes before anything asks where the tensor lives or touches the library."""
import pytest
import torch

from dir_amd import _capi
from dir_amd import functional as F

B = 2
BAD_INIT = [torch.zeros(B, 63)]               # 63 parameters, not 64


def _fit():
    F.mano_fit([None], BAD_INIT)


def _start():
    F.mano_fit_start([None], BAD_INIT)


def _sequence():
    F.mano_fit_sequence([None], BAD_INIT, torch.tensor([0, B], dtype=torch.int32))


def _pair():
    F.mano_fit_pair([None, None], BAD_INIT * 2, torch.zeros(B, 3), [torch.zeros(20)] * 2)


@pytest.mark.parametrize('call, name', [(_fit, 'mano_fit'), (_start, 'mano_fit_start'), (_sequence, 'mano_fit_sequence'), (_pair, 'mano_fit_pair')])
def test_a_wrong_shape_is_reported_under_the_wrappers_own_name(call, name):
    with pytest.raises(_capi.DirHipError) as e:
        call()
    assert str(e.value) == '%s: init must be a contiguous float32 [%d, 64] tensor on cpu' % (name, B)
