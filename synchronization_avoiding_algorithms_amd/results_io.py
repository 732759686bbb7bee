"""Result artefacts with the reference's names and logical layout.

The reference stores trajectories as HDF5 datasets ``Displacement`` of shape ``(n_dof_local, n_saved)``
(``Data_prepare.py:243-246``, ``Shared_extraction.py:38-40``, ``Online_predictor.py:321-324``).  ``h5py`` is
used when importable; else the HDF5 C library itself through ctypes (:mod:`hdf5_c`: the same container, chunked and
deflated the way ``h5py`` does it for ``compression='gzip'``); only where neither exists does the same array go to
``<name>.npz`` under the same key.  Readers accept whatever is there."""
from __future__ import annotations

import os

import numpy as np

DATASET = "Displacement"
ENERGY_DATASET = "Energy"  # the (n_rows, 5) table of drivers dynamics --energy: T, U_{n+1/2}, U_n, W, D


def _h5py():
    try:
        import h5py  # noqa: PLC0415

        return h5py
    except ImportError:
        return None


def save_displacement(path_hdf5: str, data: np.ndarray, compress: bool = True, dataset: str = DATASET) -> str:
    """Write ``data`` under ``Displacement`` (or ``dataset``); returns the path actually written."""
    os.makedirs(os.path.dirname(path_hdf5) or ".", exist_ok=True)
    h5 = _h5py()
    if h5 is not None:
        with h5.File(path_hdf5, "w") as f:
            f.create_dataset(dataset, data=data, compression="gzip" if compress else None)
        return path_hdf5
    from . import hdf5_c

    if hdf5_c.available():
        return hdf5_c.write_dataset(path_hdf5, dataset, data, gzip=compress)
    alt = os.path.splitext(path_hdf5)[0] + ".npz"
    (np.savez_compressed if compress else np.savez)(alt, **{dataset: data})
    return alt


def load_displacement(path_hdf5: str, dataset: str = DATASET) -> np.ndarray:
    h5 = _h5py()
    if os.path.exists(path_hdf5) and h5 is not None:
        with h5.File(path_hdf5, "r") as f:
            return np.array(f[dataset])
    if os.path.exists(path_hdf5):
        from . import hdf5_c

        if hdf5_c.available():
            return hdf5_c.read_dataset(path_hdf5, dataset)
    alt = os.path.splitext(path_hdf5)[0] + ".npz"
    if os.path.exists(alt):
        with np.load(alt, allow_pickle=False) as z:
            return z[dataset]
    raise FileNotFoundError(f"neither {path_hdf5} (needs h5py or libhdf5) nor {alt} exists")


def save_int_list(path: str, values) -> None:
    """``np.savetxt(..., fmt='%d')`` like ``Data_prepare.py:116-118,124``."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savetxt(path, np.asarray(values, dtype=np.int64), delimiter=",", fmt="%d")


def load_int_list(path: str) -> np.ndarray:
    return np.atleast_1d(np.genfromtxt(path, delimiter=",")).astype(np.int64)


def write_vtk_fields(path, points, cells, point_data=None, cell_data=None, title="fields"):
    """Legacy ASCII VTK of a tetrahedral mesh with named scalar ``POINT_DATA`` and ``CELL_DATA`` arrays
    (``{name: (n,) array}``, written in order), in the ``%.17g`` format of ``steady.write_vtk_point_data``.  Cells of ten
    nodes are written as quadratic tetrahedra (type 24), cells of four as type 10."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells)
    for section, data, n in (("point", point_data, len(points)), ("cell", cell_data, len(cells))):
        for name, a in (data or {}).items():
            if np.shape(a) != (n,) or not name or any(ch.isspace() for ch in name):
                raise ValueError(f"{section} data {name!r}: need a name without spaces and shape ({n},), got "
                                 f"{np.shape(a)}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(f"# vtk DataFile Version 4.2\n{title}\nASCII\nDATASET UNSTRUCTURED_GRID\n")
        fh.write(f"POINTS {len(points)} double\n")
        np.savetxt(fh, points, fmt="%.17g")
        per = cells.shape[1] if cells.ndim == 2 and cells.shape[1] == 10 else 4
        fh.write(f"CELLS {len(cells)} {(per + 1) * len(cells)}\n")
        np.savetxt(fh, np.column_stack([np.full(len(cells), per), cells]), fmt="%d")
        fh.write(f"CELL_TYPES {len(cells)}\n")
        np.savetxt(fh, np.full(len(cells), 24 if per == 10 else 10), fmt="%d")
        for section, data, n in (("POINT_DATA", point_data, len(points)), ("CELL_DATA", cell_data, len(cells))):
            if not data:
                continue
            fh.write(f"{section} {n}\n")
            for name, a in data.items():
                fh.write(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n")
                np.savetxt(fh, np.asarray(a, dtype=np.float64), fmt="%.17g")
    return path
