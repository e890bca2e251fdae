"""CPU: the host side of packed caption rows -- caption_row_lengths, the PACK_CAPTIONS switch, the validation of
`row_lengths` (before any device work), the loud failure without a device and GraphedTrainStep's refusal. The kernels and
the decoder on packed rows: tests/test_gpu_packed_rows.py."""
import pytest
import torch


def _decoder():
    from lavila_amd import gpt2_gated as G
    cfg = G.augment_gpt2_config(G.gpt2_config('gpt2', vocab_size=50, n_positions=16, n_embd=64, n_layer=1, n_head=1))
    return G.GPT2LMHeadModel(cfg).eval()


def test_caption_row_lengths():
    from lavila_amd.narrator import caption_row_lengths
    labels = torch.tensor([[5, 7, 9, 0, 0, 0],        # trailing pads
                           [5, 0, 0, 8, 0, 0],        # pad id INSIDE the caption (GPT-2's id 0 is the token "!"): stays
                           [0, 0, 0, 0, 0, 0],        # nothing but pads: one row
                           [1, 2, 3, 4, 5, 6],        # full
                           [0, 0, 0, 0, 0, 3]])       # the last position alone
    got = caption_row_lengths(labels, 0)
    assert got.dtype == torch.int64 and got.tolist() == [3, 4, 1, 6, 6]
    assert caption_row_lengths(labels, 5).tolist() == [6, 6, 6, 6, 6]          # another pad id: only trailing 5s would go
    assert caption_row_lengths(torch.full((2, 4), 9), 9).tolist() == [1, 1]


def test_pack_captions_switch_is_read_per_call(monkeypatch):
    from lavila_amd import narrator as N
    monkeypatch.setattr(N, 'PACK_CAPTIONS', None)
    monkeypatch.delenv('LAVILA_PACK_CAPTIONS', raising=False)
    assert not N.pack_captions_enabled()
    monkeypatch.setenv('LAVILA_PACK_CAPTIONS', '1')                      # read per call, not at import
    assert N.pack_captions_enabled()
    monkeypatch.setenv('LAVILA_PACK_CAPTIONS', 'true')                   # '1' alone means on
    assert not N.pack_captions_enabled()
    monkeypatch.delenv('LAVILA_PACK_CAPTIONS')
    assert not N.pack_captions_enabled()
    monkeypatch.setattr(N, 'PACK_CAPTIONS', True)
    assert N.pack_captions_enabled()
    monkeypatch.setenv('LAVILA_PACK_CAPTIONS', '1')
    monkeypatch.setattr(N, 'PACK_CAPTIONS', False)                       # the attribute, when set, decides
    assert not N.pack_captions_enabled()
    assert N.VCLM_HF.caption_pad_id == 0


@pytest.mark.parametrize('bad', [[0, 4], [4, 5], [4], [4, 4, 4], [4, 2.0], 'ab', 3,
                                 torch.tensor([0, 4]), torch.tensor([4, 5]), torch.tensor([4]), torch.tensor([[4, 4]]),
                                 torch.tensor([4.0, 4.0]), torch.tensor([True, True])])
def test_row_lengths_are_validated_before_any_device_work(bad):
    dec = _decoder()
    ids = torch.ones(2, 4, dtype=torch.long)
    with torch.no_grad(), pytest.raises(ValueError, match='row_lengths'):
        dec(ids, row_lengths=bad)


def test_packed_forward_without_a_device_is_loud_after_the_validation():
    from lavila_amd._cabi import HipExtensionError
    dec = _decoder()
    ids = torch.ones(2, 4, dtype=torch.long)
    for ok in ([4, 1], (2, 3), torch.tensor([4, 1]), torch.tensor([1, 4], dtype=torch.int32)):
        with torch.no_grad(), pytest.raises(HipExtensionError):
            dec(ids, row_lengths=ok)
    with torch.no_grad(), pytest.raises(NotImplementedError):              # it is not attention_mask, which stays refused
        dec(ids, attention_mask=torch.ones(2, 4), row_lengths=[4, 1])
    with pytest.raises(NotImplementedError, match='bf16'):                 # float32 with gradients keeps raising
        dec(ids, row_lengths=[4, 1])


def test_graphed_train_step_refuses_packed_captions(monkeypatch):
    from lavila_amd import narrator as N
    from lavila_amd.graph_step import GraphedTrainStep
    m = N.VCLM_HF.__new__(N.VCLM_HF)                                       # the refusal looks at the class and the switch only
    monkeypatch.setattr(N, 'PACK_CAPTIONS', True)
    with pytest.raises(NotImplementedError, match='LAVILA_PACK_CAPTIONS'):
        GraphedTrainStep(m, None, None, (1, 3, 1, 8, 8), (1, 77), 'cpu')
    monkeypatch.setattr(N, 'PACK_CAPTIONS', None)
    monkeypatch.setenv('LAVILA_PACK_CAPTIONS', '1')
    with pytest.raises(NotImplementedError, match='LAVILA_PACK_CAPTIONS'):
        GraphedTrainStep(m, None, None, (1, 3, 1, 8, 8), (1, 77), 'cpu')
    monkeypatch.setattr(N, 'PACK_CAPTIONS', False)                         # off: whatever is refused now is not the packing
    with pytest.raises(Exception) as e:
        GraphedTrainStep(m, None, None, (1, 3, 1, 8, 8), (1, 77), 'cpu')
    assert 'LAVILA_PACK_CAPTIONS' not in str(e.value)
