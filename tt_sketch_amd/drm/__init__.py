from .dense_gaussian_drm import DenseGaussianDRM, LazyGaussian, LazyGaussianDRM
from .khatri_rao_drm import KhatriRaoDRM
from .sparse_gaussian_drm import SparseGaussianDRM
from .sparse_sign_drm import SparseSignDRM
from .tensor_train_drm import TensorTrainDRM

# the DRMs of the reference (its test matrix runs over every pair of them); KhatriRaoDRM and LazyGaussianDRM (the
# DenseGaussianDRM that stores nothing) are this package's own
ALL_DRM = (DenseGaussianDRM, SparseGaussianDRM, TensorTrainDRM, SparseSignDRM)
