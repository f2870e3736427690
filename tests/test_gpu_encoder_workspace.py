"""-m gpu: one encoder handle serving a small request, a larger one that makes its workspace grow, and the small one again (csrc/svi_encoder_host.h
svi_enc_carve: the buffer list measured, the workspace grown, the same list carved).  The first and the third result are the same bits, and each is what a
fresh handle gives for that request alone — a carve that disagreed with its measure, or a stale pointer into the freed workspace, shows as a difference."""
import pytest
import torch

import synth
import wav2vec_cases as wc

pytestmark = pytest.mark.gpu


def _t5():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.t5_state_dict(synth.T5_SEED, **synth.T5_TINY).items()}
    make = lambda: svi_hip.WanTextEncoder.from_state_dict(sd)                                       # noqa: E731

    def request(rows):                                                                              # rows = L = valid tokens
        ids, mask = synth.t5_ids(960 + rows, rows, rows, synth.T5_TINY["vocab"])
        return lambda m: m.forward(torch.from_numpy(ids), torch.from_numpy(mask))
    return make, request(8), request(40)


def _clip():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(synth.CLIP_SEED, **synth.CLIP_TINY).items()}
    make = lambda: svi_hip.WanImageEncoder.from_state_dict(sd, num_heads=synth.CLIP_TINY["num_heads"])   # noqa: E731
    # the image encoder's workspace holds one image's buffers whatever the batch: the batch of two walks the same carve twice
    one, two = torch.from_numpy(synth.clip_image(961, 1, 3, 40, 56)), torch.from_numpy(synth.clip_image(962, 2, 3, 28, 28))
    return make, (lambda m: m.encode_image([one])), (lambda m: m.encode_image([two]))


def _w2v():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY).items()}
    make = lambda: svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(wc.TINY))              # noqa: E731
    short, long_ = wc.waveform(963, 8000), wc.waveform(964, 32000)                                  # 0.5 s and 2 s
    return make, (lambda m: m.encode(short)), (lambda m: m.encode(long_))


@pytest.mark.parametrize("case", [_t5, _clip, _w2v], ids=["t5", "clip", "w2v"])
def test_small_large_small_on_one_handle_equals_fresh_handles(case):
    make, small, large = case()
    m = make()
    first, grown, third = small(m).clone(), large(m).clone(), small(m).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(first.float()).all()) and bool(torch.isfinite(grown.float()).all())
    assert torch.equal(first, third)
    assert torch.equal(first, small(make())) and torch.equal(grown, large(make()))
