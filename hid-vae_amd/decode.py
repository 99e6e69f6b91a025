"""Constrained beam search over a tokenised corpus: the loop of the reference's stage-2 decoder (modules/model.py:165-320,
generate_next_sem_id) around HSemanticIdTokenizer.beam_step.  The model stays the caller's: `step_logits` is all this file knows of
it, and nothing of the transformer, its KV cache or its encoder cache lives here."""
from typing import Callable, NamedTuple, Optional

import torch
from torch import Tensor

from .modules.tokenizer.h_semids import BeamStep, HSemanticIdTokenizer  # noqa: F401  (BeamStep: what a step returns)


class GenerationOutput(NamedTuple):  # (modules/model.py:36-38)
    sem_ids: Tensor
    log_probas: Tensor


@torch.no_grad()
def constrained_beam_search(step_logits: Callable[[Optional[Tensor]], Tensor], tokenizer: HSemanticIdTokenizer, n_positions: int,
                            k: int = 32, n_candidates: Optional[int] = 200, temperature: float = 1.0,
                            generator: Optional[torch.Generator] = None) -> GenerationOutput:
    """step_logits(generated) -> logits [B * k_prev, V]: the caller's model on the beams so far (generated: None at position 0, then
    [B, k, i] int64, the rows of one batch item adjacent).  Each position draws n_candidates ids per row from softmax(logits /
    temperature) with torch.multinomial, as the reference does (n_candidates=None: every id is a candidate, the exhaustive step), and
    keeps the k best valid continuations with tokenizer.beam_step.  -> (sem_ids [B, k, n_positions], log_probas [B, k]), squeezed
    as the reference's GenerationOutput is."""
    if n_positions < 1:
        raise ValueError(f"constrained_beam_search: n_positions = {n_positions} (>= 1)")
    if n_candidates is not None and n_candidates < 1:
        raise ValueError(f"constrained_beam_search: n_candidates = {n_candidates} (>= 1, or None for every id)")
    generated = log_probas = None
    for _ in range(n_positions):
        logits = step_logits(generated)
        candidates = None
        if n_candidates is not None:
            probas = torch.softmax(logits / temperature, dim=-1)
            candidates = torch.multinomial(probas, num_samples=n_candidates, generator=generator)
        step = tokenizer.beam_step(logits, candidates, generated, log_probas, k=k, temperature=temperature)
        generated, log_probas = step.sem_ids, step.log_probas
    return GenerationOutput(sem_ids=generated.squeeze(), log_probas=log_probas.squeeze())
