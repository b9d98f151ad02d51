"""multimodal_mvd_seg_amd -- MI355X-native (gfx950) train-step hot path of JaronTu/Multimodal_MVD_Seg.

Only what the path needs: csrc/ (hand-written HIP kernels + the C ABI of
include/mvdseg_hip.h), ops.py (autograd glue over the ABI), network.py / losses.py / optim.py / trainer.py (host-side
mirrors of the reference's plugin interface), parallel.py (RCCL data parallelism) and inference.py (sliding-window
prediction) and ensembling.py (fold / configuration ensembles).  Importing the package does
not need a GPU; running any op does, and fails loudly when libmvdseg_hip.so is missing (there is no CPU fallback).
"""
from . import _lib  # noqa: F401

__version__ = "0.1.0"

__all__ = ["nnUNetTrainerBNMI355", "nnUNetTrainerAdamMI355", "nnUNetTrainerVanillaAdamMI355",
           "nnUNetTrainerAdam1en3MI355", "nnUNetTrainerAdam3en4MI355", "nnUNetTrainerVanillaAdam1en3MI355",
           "nnUNetTrainerVanillaAdam3en4MI355", "nnUNetTrainerCosAnnealMI355", "FinalNetTrainerMI355",
           "nnUNetTrainerDiceLossMI355", "nnUNetTrainerDiceCELoss_noSmoothMI355", "nnUNetTrainerCELossMI355",
           "nnUNetTrainerTopk10LossMI355", "nnUNetTrainerTopk10LossLS01MI355", "nnUNetTrainerDiceTopK10LossMI355",
           "nnUNetTrainerDA5MI355", "nnUNetTrainerDA5_10epochsMI355", "nnUNetTrainerNoMirroringMI355",
           "nnUNetTrainerNoDAMI355", "ensembling"]


def __getattr__(name):
    # the trainer variants a user names on the command line (nnUNetTrainerBN, nnUNetTrainerAdam, ...); resolved on first use
    # so that importing the package stays as light as before
    if name == "ensembling":
        import importlib
        return importlib.import_module(".ensembling", __name__)
    if name in __all__:
        from . import trainer
        return getattr(trainer, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
