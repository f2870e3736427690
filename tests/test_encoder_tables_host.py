"""The three encoders' weight tables without a GPU (csrc/svi_encoder_host.h EncTable behind svi_{t5,clip,w2v}_bind_weight / _check_bound): the same
refusals, in the same order, with each encoder's noun, on the tiny configurations of the case files.  Pointers are made up and aligned: binding records
them, it never reads them."""
import ctypes as C

import pytest

import encoder_kernel_cases as ek
import synth
import wav2vec_cases as wc
from svi_hip import _lib as L

OK, INVALID, UNBOUND = 0, 1, 2
PTR = 0x10000


def _t5(shared_pos=False):
    cfg = dict(ek.T5_CONFIGS["keys"], num_layers=2, shared_pos=shared_pos)
    c = L.T5Config(cfg["vocab"], cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"], cfg["num_heads"], cfg["num_layers"], cfg["num_buckets"], 128, int(shared_pos))
    return c, dict(synth.t5_param_shapes(**cfg))


def _clip():
    cfg = dict(ek.CLIP_CASES[0][1])                                       # three blocks, two of them used
    c = L.ClipConfig(cfg["image_size"], cfg["patch_size"], cfg["dim"], cfg["mlp_ratio"], cfg["num_heads"], cfg["num_layers"], cfg["num_layers"] - 1, 1e-5)
    return c, dict(synth.clip_param_shapes(**cfg))


def _w2v():
    cfg = wc.TINY
    c = L.W2vConfig(cfg["conv_dim"], cfg["hidden"], cfg["ffn"], cfg["num_heads"], cfg["num_layers"], cfg["pos_kernel"], cfg["pos_groups"], cfg["eps"])
    sh = wc.shapes(cfg)
    sh["encoder.pos_conv_embed.conv.weight"] = sh.pop(wc.PV)
    sh.pop(wc.PG)
    sh["masked_spec_embed"] = (cfg["hidden"],)
    return c, sh


# abi, noun, dtype, the other dtype, config + state-dict shapes, accepted-and-unused names, (first, last, a last-layer) key of check_bound's order
ENCODERS = {
    "t5": ("t5", "text encoder", L.SVI_BF16, L.SVI_F32, _t5, (),
           ("token_embedding.weight", "blocks.1.pos_embedding.embedding.weight", "blocks.1.attn.o.weight")),
    "clip": ("clip", "image encoder", L.SVI_F32, L.SVI_BF16, _clip,
             ("post_norm.weight", "post_norm.bias", "head", "transformer.2.mlp.0.weight"),
             ("patch_embedding.weight", "transformer.1.mlp.2.bias", "transformer.1.attn.to_qkv.weight")),
    "w2v": ("w2v", "audio encoder", L.SVI_F32, L.SVI_BF16, _w2v, ("masked_spec_embed",),
            ("feature_extractor.conv_layers.0.conv.weight", "encoder.layers.1.final_layer_norm.bias", "encoder.layers.1.layer_norm.weight")),
}


class Handle:
    def __init__(self, abi, cfg):
        self.lib, self.abi, self.h = L.lib(), abi, C.c_void_p()
        assert getattr(self.lib, f"svi_{abi}_create")(C.byref(cfg), C.byref(self.h)) == OK, L.last_error()

    def bind(self, name, shape, dtype, ptr=PTR):
        arr = (C.c_int64 * max(len(shape), 1))(*shape)
        return getattr(self.lib, f"svi_{self.abi}_bind_weight")(self.h, name.encode(), ptr, dtype, arr, len(shape))

    def check(self):
        return getattr(self.lib, f"svi_{self.abi}_check_bound")(self.h)

    def close(self):
        getattr(self.lib, f"svi_{self.abi}_destroy")(self.h)


@pytest.fixture(params=list(ENCODERS))
def enc(request):
    abi, noun, dtype, other, make, unused, keys = ENCODERS[request.param]
    cfg, shapes = make()
    h = Handle(abi, cfg)
    yield h, noun, dtype, other, shapes, unused, keys
    h.close()


def test_bind_refuses_in_order_with_the_encoders_noun(enc):
    h, noun, dtype, other, shapes, unused, keys = enc
    name = keys[2]
    shape = shapes[name]
    # dtype comes before alignment, alignment before the name, the name before the shape
    assert h.bind(name, shape, other, PTR + 4) == INVALID and noun in L.last_error() and "must be" in L.last_error()
    assert h.bind("no.such.key", shape, dtype, PTR + 4) == INVALID and "aligned" in L.last_error() and noun in L.last_error()
    assert h.bind("no.such.key", shape, dtype) == INVALID and f"unknown {noun} parameter 'no.such.key'" in L.last_error()
    wrong_rank = shape[:-1] if len(shape) > 1 else shape + (1,)
    assert h.bind(name, wrong_rank, dtype) == INVALID and f"shape mismatch for {noun} parameter '{name}'" in L.last_error()
    wrong_extent = shape[:-1] + (shape[-1] + 1,)
    assert h.bind(name, wrong_extent, dtype) == INVALID and "shape mismatch" in L.last_error() and name in L.last_error()
    assert h.bind(name, shape, dtype) == OK


def test_unused_names_are_accepted_and_not_required(enc):
    h, noun, dtype, other, shapes, unused, keys = enc
    for name in unused:
        assert h.bind(name, (7,), dtype) == OK, (name, L.last_error())                 # any shape: the parameter is never read
    for name, shape in shapes.items():
        if name not in unused:
            assert h.bind(name, shape, dtype) == OK, (name, L.last_error())
    assert h.check() == OK, L.last_error()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["first", "last", "last_layer"])
def test_check_bound_names_the_one_missing_key(enc, which):
    h, noun, dtype, other, shapes, unused, keys = enc
    missing = keys[which]
    assert h.check() == UNBOUND and f"{noun} parameter '{keys[0]}' was never bound" in L.last_error()      # nothing bound: the first key of the order
    for name, shape in shapes.items():
        if name != missing and name not in unused:
            assert h.bind(name, shape, dtype) == OK, (name, L.last_error())
    assert h.check() == UNBOUND and f"{noun} parameter '{missing}' was never bound" in L.last_error()
    assert h.bind(missing, shapes[missing], dtype) == OK and h.check() == OK


@pytest.mark.parametrize("shared", [False, True])
def test_t5_shared_pos_flips_which_position_table_is_known_and_required(shared):
    cfg, shapes = _t5(shared)
    h = Handle("t5", cfg)
    try:
        top, per = "pos_embedding.embedding.weight", "blocks.0.pos_embedding.embedding.weight"
        known, unknown = (top, per) if shared else (per, top)
        assert known in shapes and unknown not in shapes
        assert h.bind(unknown, shapes[known], L.SVI_BF16) == INVALID and "unknown text encoder parameter" in L.last_error()
        for name, shape in shapes.items():
            if name != known:
                assert h.bind(name, shape, L.SVI_BF16) == OK, (name, L.last_error())
        assert h.check() == UNBOUND and f"'{known}' was never bound" in L.last_error()
        assert h.bind(known, shapes[known], L.SVI_BF16) == OK and h.check() == OK
    finally:
        h.close()
