"""A stand-in for ``llava_next.FastDecoder`` with the REAL constructor signature, for the CPU tests that patch ``llava_next.FastDecoder``
and watch which decoders ``caption_tokens_fast(_batch)`` build: it keeps the mode record and the fields the lookup reads, and computes
nothing."""
import torch


def stand_in_decoder(built, record):
    """-> a decoder class that appends ``record(mode)`` (``mode``: its ``llava_next.CaptionMode``) to ``built`` whenever one is built."""
    from rsvld_amd import llava_next as LN

    class Dec:
        def __init__(self, model, max_len, weights="native", batch=1, prefill="torch", prefill_weights="native", release_native=False,
                     decode="valu"):
            self.mode = LN.CaptionMode(weights, prefill, prefill_weights, release_native, decode)
            self.max_len, self.batch = max_len, batch
            self.weights, self.prefill, self.prefill_weights, self.release_native, self.decode = (
                weights, prefill, prefill_weights, release_native, decode)
            built.append(record(self.mode))

        def stale(self):
            return False

        def generate(self, embeds, n, **kw):
            return torch.zeros(1, dtype=torch.long)

        def generate_batch(self, embeds, n, **kw):
            return [torch.zeros(1, dtype=torch.long) for _ in embeds]
    return Dec
