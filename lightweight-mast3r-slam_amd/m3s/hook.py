"""Run the reference's ``main.py`` UNCHANGED on the fused MI355X tracker and factor graph.

``lightweight-mast3r-slam_amd/m3s_hook/sitecustomize.py`` calls :func:`install` at interpreter start-up in every
process that has that directory on ``PYTHONPATH`` (the frontend and, through ``PYTHONPATH`` inheritance, the
spawned backend process of ``main.py``):

* when ``mast3r_slam.tracker`` / ``mast3r_slam.global_opt`` finish importing, their ``FrameTracker`` /
  ``FactorGraph`` are replaced by ``m3s.tracker.FrameTracker`` / ``m3s.global_opt.FactorGraph`` (same
  constructors, methods and returns), so ``from mast3r_slam.tracker import FrameTracker`` in ``main.py:29`` (and
  ``:17``) binds the fused classes;
* ``mast3r_slam.config.config`` becomes ``m3s.config.config`` (one dict, which the reference's ``load_config``
  updates in place: ``config.py:41-44``), so the fused classes read the YAML the run was started with;
* ``mast3r_slam.retrieval_database.RetrievalDatabase`` becomes a subclass of itself with
  ``m3s.retrieval.DatabaseMixin`` in front (``SUBCLASSES``), so ``load_retriever`` (``mast3r_utils.py:50-57``, which
  imports the name from that module) builds a database whose ``update`` runs on the device; the retrieval model and
  ``prep_features`` stay the reference's;
* ``mast3r.catmlp_dpt_head.postprocess`` becomes ``m3s.head.postprocess`` and the head class
  ``Cat_MLP_LocalFeatures_DPT_Pts3d`` a subclass of itself with ``m3s.head.FusedHeadMixin`` in front, so the head the
  model factory builds (``mast3r_head_factory`` looks both names up in that module when it is called) hands the DPT
  and MLP outputs to one HIP launch; the convolutions and the MLP stay the reference's;
* ``mast3r_slam.frame.create_frame`` becomes ``m3s.ingest.create_frame`` (``main.py:319`` calls it once per frame; it
  builds the reference's own ``Frame``): with ``M3S_INGEST_FUSED=1`` the resize, crop and normalisation run in two HIP
  launches on the uploaded camera image; with the flag unset it is the reference's host statement, bit for bit.

Nothing of the reference is copied or edited; without the hook directory on the path nothing changes.
"""
import importlib
import importlib.abc
import sys

PATCHES = {"mast3r_slam.config": ("config", "m3s.config"),
           "mast3r_slam.tracker": ("FrameTracker", "m3s.tracker"),
           "mast3r_slam.global_opt": ("FactorGraph", "m3s.global_opt"),
           "mast3r.catmlp_dpt_head": ("postprocess", "m3s.head"),
           "mast3r_slam.frame": ("create_frame", "m3s.ingest")}
# module -> (its class, the module and name of the mixin put in front of it)
SUBCLASSES = {"mast3r_slam.retrieval_database": ("RetrievalDatabase", "m3s.retrieval", "DatabaseMixin"),
              "mast3r.catmlp_dpt_head": ("Cat_MLP_LocalFeatures_DPT_Pts3d", "m3s.head", "FusedHeadMixin")}


class _PatchingFinder(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path, target=None):
        if name not in PATCHES and name not in SUBCLASSES:
            return None
        for finder in sys.meta_path:
            if finder is self or not hasattr(finder, "find_spec"):
                continue
            spec = finder.find_spec(name, path, target)
            if spec is not None:
                break
        else:
            return None
        loader = spec.loader
        orig_exec = loader.exec_module

        class _Loader(importlib.abc.Loader):
            def create_module(self, spec_):
                return loader.create_module(spec_)

            def exec_module(self, module):
                orig_exec(module)
                if name in PATCHES:
                    attr, src = PATCHES[name]
                    setattr(module, attr, getattr(importlib.import_module(src), attr))
                    setattr(module, "_m3s_original_" + attr, True)
                if name in SUBCLASSES:  # a module may have both: a name replaced and a class subclassed
                    attr, src, mixin = SUBCLASSES[name]
                    base = getattr(module, attr)
                    setattr(module, attr, type(attr, (getattr(importlib.import_module(src), mixin), base),
                                               {"__module__": base.__module__, "__doc__": base.__doc__}))
                    setattr(module, "_m3s_original_" + attr, True)

        spec.loader = _Loader()
        return spec


def install():
    """Idempotent: put the patching finder first on sys.meta_path."""
    if not any(isinstance(f, _PatchingFinder) for f in sys.meta_path):
        sys.meta_path.insert(0, _PatchingFinder())
