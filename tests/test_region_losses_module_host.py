"""CPU test that the fused loss classes stay ordinary nn.Modules: .to(), .float(), .cpu() on each class, on the
deep-supervision wrapper and on a parent module that holds one are no-ops that return the module (the losses have no
parameters), as before the label modes of DESIGN 17 were added."""
import pytest
import torch
from torch import nn

from multimodal_mvd_seg_amd import losses

KW = {'batch_dice': False, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}
MAKERS = {
    "RobustCrossEntropyLoss": lambda: losses.RobustCrossEntropyLoss(),
    "MemoryEfficientSoftDiceLoss": lambda: losses.MemoryEfficientSoftDiceLoss(),
    "DC_and_CE_loss": lambda: losses.DC_and_CE_loss(KW, {}),
    "DC_and_CE_loss(ignore_label)": lambda: losses.DC_and_CE_loss(KW, {}, ignore_label=4),
    "DC_and_BCE_loss(planes)": lambda: losses.DC_and_BCE_loss({}, KW, use_ignore_label=True),
    "DC_and_BCE_loss(regions)": lambda: losses.DC_and_BCE_loss({}, KW, regions=[(1, 2), 2]),
}


@pytest.mark.parametrize("name", list(MAKERS))
def test_module_methods_still_work(name):
    loss = MAKERS[name]()
    assert not hasattr(type(loss), '_apply') or type(loss)._apply is nn.Module._apply
    for m in (loss, losses.DeepSupervisionWrapper(loss, losses.ds_weights(3))):
        assert m.to('cpu') is m and m.float() is m and m.cpu() is m and m.to(torch.float32) is m
        assert m.train() is m and m.eval() is m

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.loss = losses.DeepSupervisionWrapper(loss, None)
            self.lin = nn.Linear(2, 2)

    h = Holder()
    assert h.to('cpu') is h and h.double().lin.weight.dtype == torch.float64 and h.float() is h
