"""The start-up hook binds the reference's ``RetrievalDatabase`` by name like the tracker and the factor graph
(m3s/hook.py SUBCLASSES): a subclass of the reference class with ``m3s.retrieval.DatabaseMixin`` in front, on a
stand-in ``mast3r_slam`` package (host test, no GPU)."""
import os
import subprocess
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightweight-mast3r-slam_amd")


def test_hook_puts_the_database_mixin_in_front_of_the_reference_class(tmp_path):
    ref = tmp_path / "ref" / "mast3r_slam"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "retrieval_database.py").write_text(textwrap.dedent("""
        class RetrievalDatabase:
            def __init__(self):
                self.kf_counter = 0
            def prep_features(self, feat):
                return "reference prep_features"
            def update(self, frame, add_after_query, k, min_thresh=0.0):
                return "reference update"
    """))
    # mast3r_utils.py:50-57 imports the name from the module, then constructs it
    (ref / "mast3r_utils.py").write_text(textwrap.dedent("""
        from mast3r_slam.retrieval_database import RetrievalDatabase
        def load_retriever():
            return RetrievalDatabase()
    """))
    main = tmp_path / "main.py"
    main.write_text(textwrap.dedent("""
        from mast3r_slam.mast3r_utils import load_retriever
        import mast3r_slam.retrieval_database as rd
        from m3s.retrieval import DatabaseMixin, QuantizeMixin
        db = load_retriever()
        assert type(db) is rd.RetrievalDatabase and type(db).__name__ == "RetrievalDatabase"
        assert isinstance(db, DatabaseMixin) and type(db).__mro__[1] is DatabaseMixin
        assert type(db).update is DatabaseMixin.update and type(db).quantize_custom is QuantizeMixin.quantize_custom
        assert db.prep_features(None) == "reference prep_features" and db.kf_counter == 0
        print("HOOK_OK")
    """))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(PKG, "m3s_hook"), PKG, str(tmp_path / "ref")]))
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "HOOK_OK" in r.stdout
    # without the hook directory the reference class stays as it is
    env["PYTHONPATH"] = os.pathsep.join([PKG, str(tmp_path / "ref")])
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "AssertionError" in r.stderr
