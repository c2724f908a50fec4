"""AsyncAmdLM's long_attention on the CPU: the constructor's checks, and that a backend whose engine has no
glb_batch_attention_tile takes the SDPA path and gives the unflagged result."""
import pytest

from tests.test_kv_chunk_cpu import _gpt2, gold  # noqa: F401  (the golden GPT-2 on the CPU restatement engine)


def test_constructor_takes_and_validates_long_attention(gold):  # noqa: F811
    assert _gpt2(gold)[0].long_attention is False and _gpt2(gold, long_attention=True)[0].long_attention is True
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError):
            _gpt2(gold, long_attention=bad)
    with pytest.raises(ValueError):
        _gpt2(gold, long_attention=True, glb_attention=False)  # the kernel is reached through the attention entry only


def test_a_flagged_forward_without_the_kernel_takes_the_sdpa_path(gold):  # noqa: F811
    (on, V), (off, _) = _gpt2(gold, long_attention=True), _gpt2(gold)
    assert not hasattr(on.engine, "batch_attention_tile")
    n = min(on.model.config.n_positions, 80)  # past SHORT_ATTENTION_MAX where the model's positions allow it
    ctxs = [[(7 * i + 3 * j) % (V - 1) + 1 for j in range(n - i)] for i in range(3)]
    assert (on.batch_next_token_logprobs_sync(ctxs) == off.batch_next_token_logprobs_sync(ctxs)).all()
