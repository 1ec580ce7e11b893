"""``python fit.py --config C --checkpoint-dir D --mesh scan.obj --landmarks
lm.json --template-landmarks idx.json --z-stats z_stats.pt --out PREFIX
[--surface] [--search {brute,grid}]``: fit a trained model to an unregistered scan (the reference's
Tester.fit_mesh, test.py:336-520) on the MI355X path
(craniofacialsd-vae_amd/fitting.py); ``--surface`` fits to the scan's
triangles instead of its vertices and reports the surface error;
``--search grid`` finds the Chamfer term's nearest neighbours through uniform
grids (dense raw scans; the same result as ``brute``, bit for bit);
``--classifiers CHECKPOINT_DIR`` also reports the fit's QDA class and its
Mahalanobis distance to the normal class."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfsd_loader  # noqa: E402

cfsd_loader.load()
from craniofacialsd_vae_amd.fitting import fit_main  # noqa: E402

if __name__ == "__main__":
    fit_main()
