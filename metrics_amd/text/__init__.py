"""Modular text metrics. Parity: torchmetrics ``text/*``.

BERTScore / InfoLM / CLIP-based metrics require user-supplied transformer
models (no weight downloads offline) — see ``metrics_amd/multimodal``.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, tensor

from metrics_amd.metric import Metric
from metrics_amd.utilities.data import dim_zero_cat
from metrics_amd.functional.text.bleu import (
    _bleu_score_compute,
    _bleu_score_update,
    chrf_score,
    translation_edit_rate,
)
from metrics_amd.functional.text.error_rates import (
    _cer_update,
    _mer_wil_wip_update,
    _norm_inputs,
    _wer_update,
    edit_distance as _edit_distance_fn,
)
from metrics_amd.functional.text.helper import get_tokenizer
from metrics_amd.functional.text.misc import (
    _perplexity_check_shapes,
    _perplexity_compute,
    _perplexity_update,
    extended_edit_distance,
    squad as _squad_fn,
)
from metrics_amd.functional.text.rouge import rouge_score


class _ErrTotalMetric(Metric):
    """Base: (errors, total) ratio metrics."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0

    errors: Tensor
    total: Tensor

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.add_state("errors", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("total", tensor(0.0), dist_reduce_fx="sum")

    def compute(self) -> Tensor:
        return self.errors / self.total

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class CharErrorRate(_ErrTotalMetric):
    """CER (stateful)."""

    def update(self, preds, target) -> None:
        """Accumulate character edits."""
        errors, total = _cer_update(preds, target)
        self.errors += errors
        self.total += total


class WordErrorRate(_ErrTotalMetric):
    """WER (stateful)."""

    def update(self, preds, target) -> None:
        """Accumulate word edits."""
        errors, total = _wer_update(preds, target)
        self.errors += errors
        self.total += total


class MatchErrorRate(_ErrTotalMetric):
    """MER (stateful)."""

    def update(self, preds, target) -> None:
        """Accumulate edits and alignment totals."""
        errors, total, _, _ = _mer_wil_wip_update(preds, target)
        self.errors += errors
        self.total += total


class WordInfoLost(Metric):
    """WIL (stateful)."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        # reference state layout (text/wip.py): errors = Σ(dist - max_len),
        # a non-positive "kept words" count — NOT backtrace hit counts
        self.add_state("errors", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("target_total", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("preds_total", tensor(0.0), dist_reduce_fx="sum")

    def update(self, preds, target) -> None:
        """Accumulate edit/length statistics."""
        errors, total, target_total, preds_total = _mer_wil_wip_update(preds, target)
        self.errors += errors - total
        self.target_total += target_total
        self.preds_total += preds_total

    def compute(self) -> Tensor:
        return 1 - (self.errors / self.target_total) * (self.errors / self.preds_total)

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class WordInfoPreserved(WordInfoLost):
    """WIP (stateful)."""

    higher_is_better = True

    def compute(self) -> Tensor:
        return (self.errors / self.target_total) * (self.errors / self.preds_total)


class EditDistance(Metric):
    """Levenshtein edit distance (stateful)."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0

    def __init__(self, substitution_cost: int = 1, reduction: str = "mean", **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if not (isinstance(substitution_cost, int) and substitution_cost >= 0):
            raise ValueError(f"Expected argument `substitution_cost` to be a positive integer, but got {substitution_cost}")
        self.substitution_cost = substitution_cost
        allowed = ("mean", "sum", "none", None)
        if reduction not in allowed:
            raise ValueError(f"Expected argument `reduction` to be one of {allowed}, but got {reduction}")
        self.reduction = reduction

        if self.reduction == "none" or self.reduction is None:
            self.add_state("edit_scores_list", default=[], dist_reduce_fx="cat")
        else:
            self.add_state("edit_scores", default=torch.tensor(0), dist_reduce_fx="sum")
            self.add_state("num_elements", default=torch.tensor(0), dist_reduce_fx="sum")

    def update(self, preds, target) -> None:
        """Accumulate per-pair edit distances."""
        scores = _edit_distance_fn(preds, target, self.substitution_cost, reduction="none")
        if self.reduction == "none" or self.reduction is None:
            self.edit_scores_list.append(scores)
        else:
            self.edit_scores += scores.sum()
            self.num_elements += scores.shape[0]

    def compute(self) -> Tensor:
        if self.reduction == "none" or self.reduction is None:
            scores = dim_zero_cat(self.edit_scores_list)
            return scores if scores.numel() else torch.tensor(0, dtype=torch.int32)
        if self.num_elements == 0:
            return torch.tensor(0, dtype=torch.int32)
        if self.reduction == "mean":
            return self.edit_scores / self.num_elements
        return self.edit_scores

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class BLEUScore(Metric):
    """BLEU (stateful)."""

    is_differentiable = False
    higher_is_better = True
    full_state_update = True
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    preds_len: Tensor
    target_len: Tensor
    numerator: Tensor
    denominator: Tensor

    def __init__(
        self, n_gram: int = 4, smooth: bool = False, weights: Optional[Sequence[float]] = None, **kwargs: Any
    ) -> None:
        super().__init__(**kwargs)
        self.n_gram = n_gram
        self.smooth = smooth
        if weights is not None and len(weights) != n_gram:
            raise ValueError(f"List of weights has different weights than `n_gram`: {len(weights)} != {n_gram}")
        self.weights = weights if weights is not None else [1.0 / n_gram] * n_gram

        self.add_state("preds_len", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("target_len", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("numerator", torch.zeros(self.n_gram), dist_reduce_fx="sum")
        self.add_state("denominator", torch.zeros(self.n_gram), dist_reduce_fx="sum")

    def _tokenize(self, s: str) -> List[str]:
        return s.split()

    def update(self, preds: Sequence[str], target: Sequence[Union[str, Sequence[str]]]) -> None:
        """Accumulate clipped n-gram counts."""
        preds_ = [preds] if isinstance(preds, str) else list(preds)
        target_ = [[t] if isinstance(t, str) else list(t) for t in target]
        p_tok = [self._tokenize(p) for p in preds_]
        t_tok = [[self._tokenize(r) for r in refs] for refs in target_]
        pl, tl = _bleu_score_update(p_tok, t_tok, self.numerator, self.denominator, self.n_gram)
        self.preds_len += pl
        self.target_len += tl

    def compute(self) -> Tensor:
        """Corpus BLEU."""
        return _bleu_score_compute(
            self.preds_len, self.target_len, self.numerator, self.denominator, self.n_gram, self.weights, self.smooth
        )

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class SacreBLEUScore(BLEUScore):
    """SacreBLEU (stateful; canonical tokenizer)."""

    def __init__(
        self,
        n_gram: int = 4,
        smooth: bool = False,
        tokenize: str = "13a",
        lowercase: bool = False,
        weights: Optional[Sequence[float]] = None,
        **kwargs: Any,
    ) -> None:
        super().__init__(n_gram=n_gram, smooth=smooth, weights=weights, **kwargs)
        self.tokenizer_fn = get_tokenizer(tokenize)
        self.lowercase = lowercase

    def _tokenize(self, s: str) -> List[str]:
        return self.tokenizer_fn(s, self.lowercase)


class CHRFScore(Metric):
    """chrF(++) (stateful; accumulates raw strings via list states of per-batch stats)."""

    is_differentiable = False
    higher_is_better = True
    full_state_update = True
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    def __init__(
        self,
        n_char_order: int = 6,
        n_word_order: int = 2,
        beta: float = 2.0,
        lowercase: bool = False,
        whitespace: bool = False,
        return_sentence_level_score: bool = False,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if not isinstance(n_char_order, int) or n_char_order < 1:
            raise ValueError("Expected argument `n_char_order` to be an integer greater than or equal to 1.")
        if not isinstance(n_word_order, int) or n_word_order < 0:
            raise ValueError("Expected argument `n_word_order` to be an integer greater than or equal to 0.")
        if beta < 0:
            raise ValueError("Expected argument `beta` to be greater than 0.")
        self.n_char_order = n_char_order
        self.n_word_order = n_word_order
        self.beta = beta
        self.lowercase = lowercase
        self.whitespace = whitespace
        self.return_sentence_level_score = return_sentence_level_score

        # reference state layout (text/chrf.py): one scalar per
        # (matching|preds|target) x (char 1..n_char, word 1..n_word)
        for kind in ("matching", "preds", "target"):
            for n in range(1, n_char_order + 1):
                self.add_state(f"total_{kind}_char_{n}_grams", tensor(0.0), dist_reduce_fx="sum")
            for n in range(1, n_word_order + 1):
                self.add_state(f"total_{kind}_word_{n}_grams", tensor(0.0), dist_reduce_fx="sum")
        if return_sentence_level_score:
            self.add_state("sentence_chrf_score", [], dist_reduce_fx="cat")

    def update(self, preds: Sequence[str], target: Sequence[Sequence[str]]) -> None:
        """Accumulate n-gram statistics (best reference per sentence)."""
        from metrics_amd.functional.text.bleu import _chrf_f_score, _ngrams

        preds_ = [preds] if isinstance(preds, str) else list(preds)
        target_ = [[t] if isinstance(t, str) else list(t) for t in target]
        total_orders = self.n_char_order + self.n_word_order

        def _prep_char(s: str) -> str:
            if self.lowercase:
                s = s.lower()
            if not self.whitespace:
                s = "".join(s.split())
            return s

        def _prep_words(s: str):
            if self.lowercase:
                s = s.lower()
            return s.split()

        for p, refs in zip(preds_, target_):
            best_f = tensor(0.0)
            best_stats = None
            for ref in refs:
                tp = torch.zeros(total_orders)
                fp = torch.zeros(total_orders)
                fn = torch.zeros(total_orders)
                p_chars, r_chars = _prep_char(p), _prep_char(ref)
                for n in range(1, self.n_char_order + 1):
                    png = _ngrams(list(p_chars), n)
                    rng = _ngrams(list(r_chars), n)
                    overlap = sum((png & rng).values())
                    tp[n - 1] = overlap
                    fp[n - 1] = sum(png.values()) - overlap
                    fn[n - 1] = sum(rng.values()) - overlap
                p_words, r_words = _prep_words(p), _prep_words(ref)
                for n in range(1, self.n_word_order + 1):
                    png = _ngrams(p_words, n)
                    rng = _ngrams(r_words, n)
                    overlap = sum((png & rng).values())
                    i = self.n_char_order + n - 1
                    tp[i] = overlap
                    fp[i] = sum(png.values()) - overlap
                    fn[i] = sum(rng.values()) - overlap
                f = _chrf_f_score(tp, fp, fn, self.beta)
                if best_stats is None or f >= best_f:
                    best_f = f
                    best_stats = (tp, fp, fn)
            tp_b, fp_b, fn_b = best_stats
            for i, name in enumerate(self._order_names()):
                setattr(self, f"total_matching_{name}", getattr(self, f"total_matching_{name}") + tp_b[i])
                setattr(self, f"total_preds_{name}", getattr(self, f"total_preds_{name}") + tp_b[i] + fp_b[i])
                setattr(self, f"total_target_{name}", getattr(self, f"total_target_{name}") + tp_b[i] + fn_b[i])
            if self.return_sentence_level_score:
                self.sentence_chrf_score.append(best_f.reshape(1))

    def _order_names(self):
        return [f"char_{n}_grams" for n in range(1, self.n_char_order + 1)] + [
            f"word_{n}_grams" for n in range(1, self.n_word_order + 1)
        ]

    def compute(self):
        """Corpus chrF from the per-order count states."""
        from metrics_amd.functional.text.bleu import _chrf_f_score

        names = self._order_names()
        tp = torch.stack([getattr(self, f"total_matching_{n}") for n in names])
        fp = torch.stack([getattr(self, f"total_preds_{n}") for n in names]) - tp
        fn = torch.stack([getattr(self, f"total_target_{n}") for n in names]) - tp
        score = _chrf_f_score(tp, fp, fn, self.beta)
        if self.return_sentence_level_score:
            return score, dim_zero_cat(self.sentence_chrf_score)
        return score

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class TranslationEditRate(Metric):
    """TER (stateful)."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0

    def __init__(
        self,
        normalize: bool = False,
        no_punctuation: bool = False,
        lowercase: bool = True,
        asian_support: bool = False,
        return_sentence_level_score: bool = False,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        self.normalize = normalize
        self.no_punctuation = no_punctuation
        self.lowercase = lowercase
        self.asian_support = asian_support
        self.return_sentence_level_score = return_sentence_level_score
        self.add_state("total_num_edits", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("total_tgt_len", tensor(0.0), dist_reduce_fx="sum")
        if return_sentence_level_score:
            self.add_state("sentence_ter", [], dist_reduce_fx="cat")

    def update(self, preds, target) -> None:
        """Accumulate edit counts."""
        score, sent = translation_edit_rate(
            preds, target, self.normalize, self.no_punctuation, self.lowercase, self.asian_support,
            return_sentence_level_score=True,
        )
        # re-derive totals: translation_edit_rate returns edits/len; recompute raw
        preds_ = [preds] if isinstance(preds, str) else list(preds)
        target_ = [[t] if isinstance(t, str) else list(t) for t in target]
        # accumulate via the sentence-level scores and lengths
        import re as _re

        def _norm(s: str):
            if self.lowercase:
                s = s.lower()
            if self.no_punctuation:
                s = _re.sub(r"[\.,\?:;!\"\(\)]", "", s)
            if self.normalize:
                s = _re.sub(r"([\.,\?:;!\"\(\)])", r" \1 ", s)
            return s.split()

        for p, refs, s_ter in zip(preds_, target_, sent):
            avg_len = sum(len(_norm(r)) for r in refs) / len(refs)
            self.total_num_edits += s_ter * avg_len
            self.total_tgt_len += avg_len
            if self.return_sentence_level_score:
                self.sentence_ter.append(s_ter.reshape(1))

    def compute(self):
        """Corpus TER."""
        score = self.total_num_edits / self.total_tgt_len
        if self.return_sentence_level_score:
            return score, dim_zero_cat(self.sentence_ter)
        return score

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class ExtendedEditDistance(Metric):
    """EED (stateful)."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    def __init__(
        self,
        language: str = "en",
        return_sentence_level_score: bool = False,
        alpha: float = 2.0,
        rho: float = 0.3,
        deletion: float = 0.2,
        insertion: float = 1.0,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if language not in ("en", "ja"):
            raise ValueError(f"Expected argument `language` to either be `en` or `ja` but got {language}")
        self.language = language
        self.return_sentence_level_score = return_sentence_level_score
        for name, val in (("alpha", alpha), ("rho", rho), ("deletion", deletion), ("insertion", insertion)):
            if not isinstance(val, float) or val < 0:
                raise ValueError(f"Parameter `{name}` is expected to be a non-negative float.")
        self.alpha = alpha
        self.rho = rho
        self.deletion = deletion
        self.insertion = insertion

        self.add_state("sentence_eed", [], dist_reduce_fx="cat")

    def update(self, preds, target) -> None:
        """Accumulate per-sentence EED."""
        _, sent = extended_edit_distance(
            preds, target, self.language, True, self.alpha, self.rho, self.deletion, self.insertion
        )
        self.sentence_eed.append(sent)

    def compute(self):
        """Average EED."""
        scores = dim_zero_cat(self.sentence_eed)
        if self.return_sentence_level_score:
            return scores.mean(), scores
        return scores.mean()

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class ROUGEScore(Metric):
    """ROUGE (stateful)."""

    is_differentiable = False
    higher_is_better = True
    full_state_update = False
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 1.0

    def __init__(
        self,
        use_stemmer: bool = False,
        normalizer=None,
        tokenizer=None,
        accumulate: str = "best",
        rouge_keys: Union[str, Tuple[str, ...]] = ("rouge1", "rouge2", "rougeL", "rougeLsum"),
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        from metrics_amd.functional.text.rouge import ALLOWED_ROUGE_KEYS

        if isinstance(rouge_keys, str):
            rouge_keys = (rouge_keys,)
        for key in rouge_keys:
            if key not in ALLOWED_ROUGE_KEYS:
                raise ValueError(f"Got unknown rouge key {key}. Expected to be one of {list(ALLOWED_ROUGE_KEYS)}")
        self.rouge_keys = rouge_keys
        self.use_stemmer = use_stemmer
        self.accumulate = accumulate
        for key in rouge_keys:
            for measure in ("fmeasure", "precision", "recall"):
                self.add_state(f"{key}_{measure}".replace(".", "_"), [], dist_reduce_fx="cat")

    def update(self, preds, target) -> None:
        """Accumulate per-pair ROUGE statistics."""
        preds_ = [preds] if isinstance(preds, str) else list(preds)
        if isinstance(target, str):
            target_ = [[target]]
        elif target and isinstance(target[0], str):
            target_ = [[t] for t in target]
        else:
            target_ = [list(t) for t in target]
        for p, refs in zip(preds_, target_):
            res = rouge_score([p], [refs], accumulate=self.accumulate, use_stemmer=self.use_stemmer,
                              rouge_keys=self.rouge_keys)
            for k, v in res.items():
                getattr(self, k.replace(".", "_")).append(v.reshape(1))

    def compute(self) -> Dict[str, Tensor]:
        """Mean ROUGE statistics over the corpus."""
        out = {}
        for key in self.rouge_keys:
            for measure in ("fmeasure", "precision", "recall"):
                name = f"{key}_{measure}"
                out[name] = dim_zero_cat(getattr(self, name.replace(".", "_"))).mean()
        return out

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class SQuAD(Metric):
    """SQuAD EM/F1 (stateful)."""

    is_differentiable = False
    higher_is_better = True
    full_state_update = False
    plot_lower_bound: float = 0.0
    plot_upper_bound: float = 100.0

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.add_state("f1_score", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("exact_match", tensor(0.0), dist_reduce_fx="sum")
        self.add_state("total", tensor(0, dtype=torch.int32), dist_reduce_fx="sum")

    def update(self, preds, target) -> None:
        """Accumulate EM/F1 sums."""
        from metrics_amd.functional.text.misc import _squad_em, _squad_f1

        if isinstance(preds, dict):
            preds = [preds]
        if isinstance(target, dict):
            target = [target]
        pred_by_id = {p["id"]: p["prediction_text"] for p in preds}
        for t in target:
            tid = t["id"]
            if tid not in pred_by_id:
                continue
            answers = t["answers"]["text"]
            self.f1_score += max(_squad_f1(pred_by_id[tid], a) for a in answers)
            self.exact_match += max(_squad_em(pred_by_id[tid], a) for a in answers)
            self.total += 1

    def compute(self) -> Dict[str, Tensor]:
        return {
            "exact_match": 100.0 * self.exact_match / self.total,
            "f1": 100.0 * self.f1_score / self.total,
        }

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class Perplexity(Metric):
    """Perplexity (stateful)."""

    is_differentiable = True
    higher_is_better = False
    full_state_update = False
    plot_lower_bound: float = 0.0

    total_log_probs: Tensor
    count: Tensor

    def __init__(self, ignore_index: Optional[int] = None, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if ignore_index is not None and not isinstance(ignore_index, int):
            raise ValueError(f"Argument `ignore_index` expected to either be `None` or an `int` but got {ignore_index}")
        self.ignore_index = ignore_index
        self.add_state("total_log_probs", default=tensor(0.0), dist_reduce_fx="sum")
        self.add_state("count", default=tensor(0.0), dist_reduce_fx="sum")

    def update(self, preds: Tensor, target: Tensor) -> None:
        """Accumulate total NLL + token count."""
        if preds.is_cuda:
            # GPU: the kernel adds into the two states in place, no host sync
            from metrics_amd.ops import _hip

            _perplexity_check_shapes(preds, target)
            if _hip.lm_nll_into(preds, target, self.ignore_index, self.total_log_probs, self.count, owner=self):
                return
        total, count = _perplexity_update(preds, target, self.ignore_index)
        self.total_log_probs += total
        self.count += count

    def compute(self) -> Tensor:
        return _perplexity_compute(self.total_log_probs, self.count)

    def plot(self, val=None, ax=None):
        return self._plot(val, ax)


class BERTScore(Metric):
    """BERTScore with a user-supplied transformer encoder + tokenizer.

    Greedy cosine matching of contextual embeddings (precision/recall/f1).
    The reference downloads a model by name; offline, pass ``model=`` and
    ``user_tokenizer=`` (HuggingFace-style, from a local path).
    """

    is_differentiable = False
    higher_is_better = True
    full_state_update = False

    def __init__(
        self,
        model_name_or_path: Optional[str] = None,
        num_layers: Optional[int] = None,
        all_layers: bool = False,
        model=None,
        user_tokenizer=None,
        user_forward_fn=None,
        verbose: bool = False,
        idf: bool = False,
        device=None,
        max_length: int = 512,
        batch_size: int = 64,
        num_threads: int = 0,
        return_hash: bool = False,
        lang: str = "en",
        rescale_with_baseline: bool = False,
        baseline_path: Optional[str] = None,
        baseline_url: Optional[str] = None,
        truncation: bool = False,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if model is None or user_tokenizer is None:
            raise ModuleNotFoundError(
                "BERTScore needs a local transformer model + tokenizer: pass `model=` and `user_tokenizer=`"
                " (weights cannot be downloaded in this offline environment)."
            )
        # reference-parity knobs that require online artifacts are rejected
        # loudly instead of silently ignored
        if idf:
            raise NotImplementedError(
                "BERTScore(idf=True) is not supported offline (cannot be validated without real model weights)."
            )
        if rescale_with_baseline:
            raise NotImplementedError(
                "BERTScore(rescale_with_baseline=True) needs baseline files that cannot be fetched offline."
            )
        if return_hash:
            raise NotImplementedError("BERTScore(return_hash=True) refers to a downloaded-model hash (offline N/A).")
        self.model = model
        self.tokenizer = user_tokenizer
        self.user_forward_fn = user_forward_fn
        self.verbose = verbose
        self.lang = lang
        self.truncation = truncation
        self.max_length = max_length
        self.batch_size = batch_size
        if num_threads:
            import torch as _torch

            _torch.set_num_threads(num_threads)
        if device is not None:
            self.model = self.model.to(device)
        self.model.eval()
        self.add_state("precision_scores", [], dist_reduce_fx="cat")
        self.add_state("recall_scores", [], dist_reduce_fx="cat")
        self.add_state("f1_scores", [], dist_reduce_fx="cat")

    @torch.no_grad()
    def _embed(self, texts: List[str]):
        enc = self.tokenizer(
            texts, return_tensors="pt", padding=True, truncation=self.truncation or True,
            max_length=self.max_length,
        )
        if self.user_forward_fn is not None:
            out = self.user_forward_fn(self.model, enc)
        else:
            out = self.model(**enc)
        emb = out.last_hidden_state if hasattr(out, "last_hidden_state") else out[0]
        mask = enc["attention_mask"].bool()
        emb = emb / emb.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        return emb, mask

    def update(self, preds: List[str], target: List[str]) -> None:
        """Greedy-match contextual embeddings per pair."""
        if isinstance(preds, str):
            preds = [preds]
        if isinstance(target, str):
            target = [target]
        p_emb, p_mask = self._embed(list(preds))
        t_emb, t_mask = self._embed(list(target))
        for i in range(len(preds)):
            pe = p_emb[i][p_mask[i]]
            te = t_emb[i][t_mask[i]]
            sim = pe @ te.t()
            precision = sim.max(dim=1).values.mean()
            recall = sim.max(dim=0).values.mean()
            f1 = 2 * precision * recall / (precision + recall + 1e-12)
            self.precision_scores.append(precision.reshape(1))
            self.recall_scores.append(recall.reshape(1))
            self.f1_scores.append(f1.reshape(1))

    def compute(self) -> Dict[str, Tensor]:
        return {
            "precision": dim_zero_cat(self.precision_scores),
            "recall": dim_zero_cat(self.recall_scores),
            "f1": dim_zero_cat(self.f1_scores),
        }


class InfoLM(Metric):
    """InfoLM: information measures between masked-LM distributions.

    Requires a user-supplied masked language model + tokenizer (offline).
    """

    is_differentiable = False
    higher_is_better = False
    full_state_update = False

    def __init__(
        self,
        model_name_or_path: str = "bert-base-uncased",
        temperature: float = 0.25,
        information_measure: str = "kl_divergence",
        idf: bool = True,
        alpha: Optional[float] = None,
        beta: Optional[float] = None,
        device=None,
        max_length: Optional[int] = None,
        batch_size: int = 64,
        num_threads: int = 0,
        verbose: bool = True,
        return_sentence_level_score: bool = False,
        model=None,
        user_tokenizer=None,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if model is None or user_tokenizer is None:
            raise ModuleNotFoundError(
                "InfoLM needs a local masked LM + tokenizer: pass `model=` and `user_tokenizer=`"
                " (weights cannot be downloaded in this offline environment)."
            )
        allowed = ("kl_divergence", "alpha_divergence", "beta_divergence", "ab_divergence",
                   "renyi_divergence", "l1_distance", "l2_distance", "l_infinity_distance", "fisher_rao_distance")
        if information_measure not in allowed:
            raise ValueError(f"Argument `information_measure` expected one of {allowed}")
        if information_measure in ("alpha_divergence", "ab_divergence", "renyi_divergence") and alpha is None:
            raise ValueError(f"Argument `alpha` is required for information_measure={information_measure}")
        if information_measure in ("beta_divergence", "ab_divergence") and beta is None:
            raise ValueError(f"Argument `beta` is required for information_measure={information_measure}")
        self.model = model
        self.tokenizer = user_tokenizer
        self.temperature = temperature
        self.information_measure = information_measure
        self.idf = idf
        self.alpha = alpha
        self.beta = beta
        self.max_length = max_length
        self.batch_size = batch_size
        self.verbose = verbose
        self.return_sentence_level_score = return_sentence_level_score
        if num_threads:
            import torch as _torch

            _torch.set_num_threads(num_threads)
        if device is not None:
            self.model = self.model.to(device)
        self.model.eval()
        self.add_state("scores", [], dist_reduce_fx="cat")

    @torch.no_grad()
    def _dist(self, texts: List[str]) -> Tensor:
        enc = self.tokenizer(texts, return_tensors="pt", padding=True, truncation=True)
        out = self.model(**enc)
        logits = out.logits if hasattr(out, "logits") else out[0]
        probs = (logits / self.temperature).softmax(-1)
        mask = enc["attention_mask"].unsqueeze(-1)
        return (probs * mask).sum(1) / mask.sum(1)

    def update(self, preds: List[str], target: List[str]) -> None:
        """Accumulate the information measure between bag-of-token MLM distributions."""
        if isinstance(preds, str):
            preds = [preds]
        if isinstance(target, str):
            target = [target]
        p = self._dist(list(preds)).clamp(min=1e-12)
        t = self._dist(list(target)).clamp(min=1e-12)
        if self.information_measure == "kl_divergence":
            score = (t * (t / p).log()).sum(-1)
        elif self.information_measure == "l1_distance":
            score = (t - p).abs().sum(-1)
        elif self.information_measure == "l2_distance":
            score = (t - p).pow(2).sum(-1).sqrt()
        elif self.information_measure == "l_infinity_distance":
            score = (t - p).abs().max(-1).values
        elif self.information_measure == "fisher_rao_distance":
            score = 2 * torch.acos(((t * p).sqrt().sum(-1)).clamp(0, 1))
        elif self.information_measure == "alpha_divergence":
            a = self.alpha
            score = (1.0 / (a * (a - 1.0))) * ((t.pow(a) * p.pow(1 - a)).sum(-1) - 1.0)
        elif self.information_measure == "beta_divergence":
            b = self.beta
            score = (
                (t.pow(b + 1).sum(-1) / (b * (b + 1)))
                + (p.pow(b + 1).sum(-1) / (b + 1))
                - ((t * p.pow(b)).sum(-1) / b)
            )
        elif self.information_measure == "ab_divergence":
            a, b = self.alpha, self.beta
            score = (
                (t.pow(a + b).sum(-1) / (b * (a + b)))
                + (p.pow(a + b).sum(-1) / (a * (a + b)))
                - ((t.pow(a) * p.pow(b)).sum(-1) / (a * b))
            )
        elif self.information_measure == "renyi_divergence":
            a = self.alpha
            score = ((t.pow(a) * p.pow(1 - a)).sum(-1)).log() / (a - 1.0)
        else:
            score = (t * (t / p).log()).sum(-1)
        self.scores.append(score)

    def compute(self):
        scores = dim_zero_cat(self.scores)
        if self.return_sentence_level_score:
            return scores.mean(), scores
        return scores.mean()


__all__ = [
    "BERTScore",
    "BLEUScore",
    "CHRFScore",
    "CharErrorRate",
    "EditDistance",
    "ExtendedEditDistance",
    "InfoLM",
    "MatchErrorRate",
    "Perplexity",
    "ROUGEScore",
    "SQuAD",
    "SacreBLEUScore",
    "TranslationEditRate",
    "WordErrorRate",
    "WordInfoLost",
    "WordInfoPreserved",
]
