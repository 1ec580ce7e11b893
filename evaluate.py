"""``python evaluate.py --id ID [--output_path P] [--precision fp32|bf16] [--seed S]
[--no-animations] [--diversity-samples N] [--only NAME[,NAME]] [--patient PATH]...
[--pairs FILE --pairs-root DIR]``: evaluate the
model trained as ``ID`` (the reference's ``python test.py --id ID``,
test.py:57-79, 1443-1480) on the MI355X path
(craniofacialsd-vae_amd/evaluation.py): latent traversals with their
per-region table, random generation, reconstruction errors and the two
diversity figures (``eval_metrics.json``) and, when the run trained
classifiers, their test reports.  Everything is written into
``<output_path>/outputs/<ID>``.  ``--only`` runs single steps: traversals,
embeddings, classifiers, generation, metrics, interpolate, tsne (the t-SNE
embedding of the train and test latents, ``tsne_embeddings.npz``; it needs no
classifiers and is not part of the whole run, as in the reference), plan
(``--patient PATH``, once per patient: the patient classified, projected and
moved to the healthy distribution, procedure by procedure, under
``interpolations/``) and prepost (``--pairs FILE --pairs-root DIR``: the
surgical-effectiveness metrics of every pre- / post-operative pair of the
table, under ``pre_post_eval/``) and figures (the embedding figures drawn on
the device, ``lda_emb_*.png`` and the region sheets, or ``tsne_emb_*.png``
without classifiers; with ``--patient`` the path to normal on them, with
``--pairs`` / ``--pairs-root`` the pre / post arrows, under
``pre_post_eval_plots/``); none of these is part of the whole run either."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfsd_loader  # noqa: E402

cfsd_loader.load()
from craniofacialsd_vae_amd.evaluation import evaluate_main  # noqa: E402

if __name__ == "__main__":
    evaluate_main()
