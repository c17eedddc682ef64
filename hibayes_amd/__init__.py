"""hibayes_amd — MI355X-native engine for hibayes' individual-level per-SNP Gibbs sampler.

Public surface mirrors the reference's for this path (YinLiLin/hibayes v3.1.0):
    ibrm()        R/bayes.r:121          read_plink()  R/read_plink.r:24
    Bayes()       src/Bayes.cpp:60       cutwind_by_bp / cutwind_by_num  src/cutwind.cpp
    sbrm()        R/sbayes.r:101         ldmat()       R/ldm.r:31
    conjgt_den() / conjgt_spa()  src/cg.cpp:4-129 (sbrm's method = "CG": sbrm_cg())
    make_grm()    src/rm.cpp:5          (ibrm's method = "BSLMM": the relationship matrix and its eigenvectors)
    eigh()        src/rm.cpp:46-52      (eigen_sym_dc: the symmetric eigen-decomposition, reduction and back-transformation on the device)
    ssbrm()       R/ssbayes.r:115       make_ped() / make_Ainv()  src/rm.cpp:56-206   (the single-step model; its epsilon block on the device)
    grm_inverse() / spd_inverse()  src/rm.cpp:39-42, src/solver.cpp:159-259 (make_grm(inverse = TRUE): solve(), Cholesky on the device, LU on the host)
    impute_device()  R/ssbayes.r:295-307 (the single-step model's imputation as a batched conjugate-gradient solve on the device)
    window_pve()  README item (8), after R/bayes.r:303-308 (the variance explained by windows of markers, per record: PVE and variance-based WPPA)
    ld_window_pve()  README item (8), after R/sbayes.r:231-234 (the same from the LD matrix of the summary-level model; sbrm(pve=True))
All compute runs in libhibayes_gpu.so (hand-written gfx950 HIP kernels behind include/hibayes_gpu.h).
"""
from ._lib import HibayesError, lib, LIB_PATH
from .bayes import Bayes, ibrm
from .sbayes import SBayesD, SBayesS, sbrm
from .cg import conjgt_den, conjgt_spa, sbrm_cg
from .engine import Context
from .ldm import LDMatrix, ldmat
from .grm import make_grm
from .eig import eigh
from .chol import chol_factor, grm_inverse, solver_lu, spd_inverse
from .ssbayes import ssbrm, ssbrm_prepare, make_ped, make_Ainv
from .impute import impute_device
from .plink import read_plink, read_table, decode_bed, attach_bigmatrix, read_bigmatrix, write_bigmatrix
from .windows import cutwind_by_bp, cutwind_by_num
from .pve import ld_window_pve, window_pve

__all__ = ["Bayes", "ibrm", "read_plink", "read_table", "decode_bed", "attach_bigmatrix", "read_bigmatrix", "write_bigmatrix", "Context", "cutwind_by_bp",
           "cutwind_by_num", "SBayesD", "SBayesS", "sbrm", "conjgt_den", "conjgt_spa", "sbrm_cg", "ldmat", "LDMatrix", "make_grm", "eigh", "grm_inverse", "spd_inverse", "solver_lu", "chol_factor", "ssbrm", "ssbrm_prepare", "make_ped", "make_Ainv", "impute_device", "window_pve", "ld_window_pve", "HibayesError", "lib", "LIB_PATH"]
__version__ = "0.1.0"
