"""Regenerate docs/PARITY.md: reference __all__ -> providing metrics_amd module."""
import ast
import importlib
import os
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SECTIONS = [
    ("torchmetrics (top level)", "", "metrics_amd"),
    ("torchmetrics.classification", "classification", "metrics_amd.classification"),
    ("torchmetrics.regression", "regression", "metrics_amd.regression"),
    ("torchmetrics.retrieval", "retrieval", "metrics_amd.retrieval"),
    ("torchmetrics.clustering", "clustering", "metrics_amd.clustering"),
    ("torchmetrics.nominal", "nominal", "metrics_amd.nominal"),
    ("torchmetrics.segmentation", "segmentation", "metrics_amd.segmentation"),
    ("torchmetrics.detection", "detection", "metrics_amd.detection"),
    ("torchmetrics.image", "image", "metrics_amd.image"),
    ("torchmetrics.audio", "audio", "metrics_amd.audio"),
    ("torchmetrics.text", "text", "metrics_amd.text"),
    ("torchmetrics.multimodal", "multimodal", "metrics_amd.multimodal"),
    ("torchmetrics.shape", "shape", "metrics_amd.shape"),
    ("torchmetrics.wrappers", "wrappers", "metrics_amd.wrappers"),
    ("torchmetrics.functional", "functional", "metrics_amd.functional"),
    ("torchmetrics.utilities", "utilities", "metrics_amd.utilities"),
]


# hand-written, appended verbatim behind the generated map
DEVIATIONS = """## Known value deviations

- Thresholding of logits. The fused binary / multilabel stat kernels test
  `x > logit(thr)` instead of `sigmoid(x) > thr` (docs/ROADMAP.md). Inside a
  fused multilabel collection plan (`_FusedMultilabelUpdatePlan`,
  docs/ARCHITECTURE.md "Fused multilabel step") the confusion-matrix and
  exact-match leaders (`MultilabelConfusionMatrix`, `MultilabelMatthewsCorrCoef`,
  `MultilabelJaccardIndex`, `MultilabelExactMatch`) get the same rule, where
  their stand-alone updates compute `sigmoid(x) > thr` in torch and, for bf16
  inputs, round the sigmoid back to bf16 before the comparison. The plan's rule
  is the exact answer to `sigmoid(x) > thr` and makes confusion matrix, exact
  match and stat scores of one collection mutually consistent; it differs from
  the torch path only in the rounding band around the cut-off
  (`0 < x < ~1e-7` for fp32 at `thr = 0.5`, a wider band for bf16).
  `METRICS_AMD_FUSE_MULTILABEL=0` keeps every leader on its own path.
- The same inside a fused binary collection plan (`_FusedBinaryUpdatePlan`,
  docs/ARCHITECTURE.md "Fused binary step"): the confusion-matrix leader
  (`BinaryConfusionMatrix`, `BinaryMatthewsCorrCoef`, `BinaryJaccardIndex`,
  `BinaryCohenKappa`) thresholds `x > logit(thr)` when its batch is normalised,
  where its stand-alone update compares `sigmoid(x)`, rounded to bf16 for bf16
  inputs, with `thr`. The two differ only inside that rounding band. Which
  batches are normalised does not change: the stat group decides over all
  elements, confusion matrix and curve over the elements that are not ignored,
  as on their own paths. `METRICS_AMD_FUSE_BINARY=0` keeps every leader on its
  own path.
- Multilabel ranking metrics on the GPU (`csrc/ml_rank.hip`,
  docs/ARCHITECTURE.md "Multilabel ranking kernel"). Coverage error and
  ranking average precision are functions of the tie classes alone and equal
  the torch path; the kernel forms every batch sum in fp64 and rounds the fp32
  state once per update, where the torch path sums rows in fp32.
  - Ranking loss, tie rule. The reference ranks with an unstable
    `argsort().argsort()`, which leaves the value open when a relevant and an
    irrelevant label of a row have the same score (bf16 sigmoids tie heavily,
    fp32 sigmoids saturate to 1.0 from about x = 17). The kernel uses the
    position under a STABLE ascending sort,
    `inv_j = #{k : s_k < s_j} + #{k < j : s_k == s_j}`, one of the outcomes the
    reference can produce. Ties
    among relevant labels only, or among irrelevant ones only, do not change
    the loss.
  - Coverage error with `ignore_index`. The reference writes `-4L` into the
    score of an ignored element and does not exclude it from the row minimum,
    so a row with at least one ignored element "covers" all L labels, whatever
    its relevant labels score. The kernel reproduces this on purpose
    (coverage = L for such a row); it is a quirk of the reference, not a
    choice of this project.
  - NaN scores. The kernel never faults and every comparison with a NaN is
    false, but the values of a row that holds one are unspecified and need not
    equal the torch path (whose `unique` and `argsort` order NaN last).
  - `METRICS_AMD_RANKING_KERNEL=0` keeps the torch path everywhere.
"""


def main() -> None:
    out = [
        "# Reference parity map",
        "",
        "Auto-generated (tools/gen_parity.py): every public symbol of the reference",
        "(torchmetrics 1.7.0dev) `__all__`, and the metrics_amd module that provides",
        "it. `MISSING` would mark a gap.",
        "",
    ]
    total = missing = 0
    body = []
    for title, sub, mymod in SECTIONS:
        path = f"/root/reference/src/torchmetrics/{sub + '/' if sub else ''}__init__.py"
        try:
            src = open(path).read()
        except FileNotFoundError:
            continue
        ref_all = None
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.Assign) and any(getattr(t, "id", "") == "__all__" for t in node.targets):
                ref_all = ast.literal_eval(node.value)
        if not ref_all:
            continue
        mine = importlib.import_module(mymod)
        body.append(f"## {title} ({len(ref_all)} symbols)")
        body.append("")
        by_mod = defaultdict(list)
        for n in sorted(ref_all):
            total += 1
            obj = getattr(mine, n, None)
            if obj is None:
                missing += 1
                body.append(f"- `{n}` — **MISSING**")
            else:
                by_mod[getattr(obj, "__module__", mymod)].append(n)
        for m in sorted(by_mod):
            body.append(f"- `{m}`: " + ", ".join(f"`{n}`" for n in by_mod[m]))
        body.append("")
    out.append(f"Coverage: {total - missing}/{total} symbols present.")
    out.append("")
    open("docs/PARITY.md", "w").write("\n".join(out + body) + "\n" + DEVIATIONS)
    print(f"{total - missing}/{total} present")


if __name__ == "__main__":
    main()
