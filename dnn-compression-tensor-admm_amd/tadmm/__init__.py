"""tadmm -- MI355X-native ADMM low-rank projection path (host-side mirror of the reference API).

Public surface mirrors the reference modules (admm.py, ttd.py, TTConv.py, TTLinear.py, TKConv.py,
TKLinear.py, SVDConv.py, StfTKConv.py, the three *Embedding.py, ablation/tt_lstm_inference.py, losses.py, the layer losses of xcompression/task_distill.py, xcompression/transformer/optimization.py, the self-attention of xcompression/transformer/compressed_modeling*.py, vit_tt.py, utils.get_hp_dict); arithmetic runs in libtadmm_hip.so (csrc/) through the C ABI of
include/tadmm.h.  Importing the package does not need a GPU; computing does, and there is no CPU
fallback: a missing library or device raises.
"""
from . import _cabi  # noqa: F401
from .hp import get_hp_dict  # noqa: F401


def __getattr__(name):
    # heavier sub-modules (they import torch.nn) are resolved lazily
    import importlib
    table = {
        "ADMM": ("admm", "ADMM"), "ten2tt": ("ttd", "ten2tt"), "tt2ten": ("ttd", "tt2ten"),
        "TTConv2dM": ("tt_layers", "TTConv2dM"), "TTConv2dR": ("tt_layers", "TTConv2dR"),
        "TTLinearM": ("tt_layers", "TTLinearM"), "TTLinearR": ("tt_layers", "TTLinearR"),
        "TKConv2dC": ("tk_layers", "TKConv2dC"), "TKConv2dM": ("tk_layers", "TKConv2dM"),
        "TKConv2dR": ("tk_layers", "TKConv2dR"), "TKLinearM": ("tk_layers", "TKLinearM"),
        "TKLinearR": ("tk_layers", "TKLinearR"),
        "SVDConv2dR": ("svd_layers", "SVDConv2dR"), "SVDConv2dC": ("svd_layers", "SVDConv2dC"),
        "SVDConv2dM": ("svd_layers", "SVDConv2dM"),
        "append_double_l2_loss": ("orthogonal", "append_double_l2_loss"),
        "StfTKConv2dC": ("stf_layers", "StfTKConv2dC"), "StiefelParameter": ("stf_layers", "StiefelParameter"),
        "StiefelSGD": ("riemannian", "StiefelSGD"), "StiefelAdam": ("riemannian", "StiefelAdam"),
        "TTEmbedding": ("emb_layers", "TTEmbedding"), "TTMEmbedding": ("emb_layers", "TTMEmbedding"),
        "SVDEmbedding": ("emb_layers", "SVDEmbedding"),
        "TTLSTM": ("rnn_layers", "TTLSTM"),
        "DistillationLoss": ("losses", "DistillationLoss"), "TinyBertLayerLoss": ("losses", "TinyBertLayerLoss"),
        "BertAdam": ("optimization", "BertAdam"),
        "BertSelfAttention": ("bert_layers", "BertSelfAttention"),
        "BertLayerNorm": ("bert_layers", "BertLayerNorm"), "BertSelfOutput": ("bert_layers", "BertSelfOutput"),
        "BertIntermediate": ("bert_layers", "BertIntermediate"), "BertOutput": ("bert_layers", "BertOutput"),
        "BertAttention": ("bert_layers", "BertAttention"), "BertLayer": ("bert_layers", "BertLayer"),
        "BertEncoder": ("bert_layers", "BertEncoder"), "BertEmbeddings": ("bert_layers", "BertEmbeddings"),
        "BertPooler": ("bert_layers", "BertPooler"),
        "stiefel_step": ("ops", "stiefel_step"), "stiefel_project_": ("ops", "stiefel_project_"),
    }
    # vit_tt.py: the modules and the twelve factories
    for attr in ("DropPath", "PatchEmbed", "TTAttention", "TTMlp", "TTBlock", "TTVisionTransformer"):
        table[attr] = ("vit_layers", attr)
    for kind in ("ttm", "ttr", "tkm", "tkr"):
        for arch in ("vit_small", "deit_tiny", "deit_small"):
            table[f"{kind}_{arch}_patch16_224"] = ("vit_layers", f"{kind}_{arch}_patch16_224")
    if name == "optimization":    # the module itself, as the reference's scripts import it
        return importlib.import_module(".optimization", __name__)
    if name in table:
        mod, attr = table[name]
        return getattr(importlib.import_module("." + mod, __name__), attr)
    raise AttributeError(name)
