"""tadmm -- MI355X-native ADMM low-rank projection path (host-side mirror of the reference API).

Public surface mirrors the reference modules (admm.py, ttd.py, TTConv.py, TTLinear.py, TKConv.py,
TKLinear.py, SVDConv.py, StfTKConv.py, the three *Embedding.py, ablation/tt_lstm_inference.py, losses.py, the layer losses of xcompression/task_distill.py, xcompression/transformer/optimization.py, the self-attention of xcompression/transformer/compressed_modeling*.py, vit_tt.py, resnet_cifar_tt.py, resnet_inet_tt.py, mobilenetv2_cifar_tt.py, mobilenetv2_tt.py, densenet_cifar_tt.py, densenet_inet_tt.py, utils.get_hp_dict); arithmetic runs in libtadmm_hip.so (csrc/) through the C ABI of
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
    # resnet_cifar_tt.py and resnet_inet_tt.py: the factories (their names do not collide); both files define TTBasicBlock
    # and TTResNet, so the classes are reached through the modules tadmm.resnet_cifar_layers / tadmm.resnet_inet_layers
    for kind, archs in (("ttr", (20, 32, 56)), ("ttm", (20, 32)), ("tkr", (20, 32, 56)), ("tkm", (20, 32)),
                        ("tkc", (20, 32)), ("stftkc", (32,))):
        for depth in archs:
            table[f"{kind}_resnet{depth}"] = ("resnet_cifar_layers", f"{kind}_resnet{depth}")
    for fn in ("ttr_resnet18", "ttm_resnet18", "tkc_resnet18", "tkm_resnet18", "ttr_resnet34", "ttr_resnet50",
               "tkr_resnet18", "tkr_resnet34", "tkr_resnet50", "tkm_resnet50", "tkc_resnet50"):
        table[fn] = ("resnet_inet_layers", fn)
    # mobilenetv2_cifar_tt.py and mobilenetv2_tt.py: the factories; both files define TTMobileNetV2, so the classes are
    # reached through the modules tadmm.mobilenet_cifar_layers / tadmm.mobilenet_inet_layers
    for kind in ("tkr", "tkc", "tkm", "svdr", "svdc", "svdm"):
        table[f"{kind}_mobilenetv2_cifar"] = ("mobilenet_cifar_layers", f"{kind}_mobilenetv2_cifar")
    for kind in ("ttr", "tkc", "svdc", "svdm"):
        table[f"{kind}_mobilenetv2"] = ("mobilenet_inet_layers", f"{kind}_mobilenetv2")
    # densenet_cifar_tt.py and densenet_inet_tt.py: the factories; both files define TenDenseBlock and TenDenseNet, so the
    # classes are reached through the modules tadmm.densenet_cifar_layers / tadmm.densenet_inet_layers
    table["tkr_densenet40"] = ("densenet_cifar_layers", "tkr_densenet40")
    for fn in ("tkc_densenet121", "tkc_densenet201", "tkc_densenet264"):
        table[fn] = ("densenet_inet_layers", fn)
    table["DenseFeatures"] = ("functional", "DenseFeatures")
    if name in ("optimization", "resnet_cifar_layers", "resnet_inet_layers", "mobilenet_cifar_layers",
                "mobilenet_inet_layers", "densenet_cifar_layers", "densenet_inet_layers"):    # the modules themselves
        return importlib.import_module("." + name, __name__)
    if name in table:
        mod, attr = table[name]
        return getattr(importlib.import_module("." + mod, __name__), attr)
    raise AttributeError(name)
