"""The lazy Gram's plan (pipeline.lazy_gram_head / gram_head_size) on a stub backend: when
the step may prune from the head block of its order, and how many rows the head has."""
import pytest

from factormodeling_amd import pipeline as PL


class _Lazy:
    """A backend with the two head entries (never called here)."""
    gram_exact_rows = prune_head = staticmethod(lambda *a, **k: None)


class _NoHead:
    pass


SIDE = {"zscore": object()}


def _head(cfg=None, be=_Lazy(), F=200, side=SIDE, collect=None, top=5):
    return PL.lazy_gram_head(cfg or PL.StepConfig(lazy_gram=True), be, F, side, collect, top)


def test_eligible_c2_shape():
    assert _head() == 32


@pytest.mark.parametrize("why,kw", [
    ("no Gram", dict(cfg=PL.StepConfig(lazy_gram=True, gram=False))),
    ("switched off", dict(cfg=PL.StepConfig(lazy_gram=False))),
    ("streams", dict(cfg=PL.StepConfig(lazy_gram=True, streams=True))),
    ("top is None (C4: the whole zoo)", dict(top=None)),
    ("top is not an integer", dict(top=5.0)),
    ("backend without the head entries", dict(be=_NoHead())),
    ("wide zoo", dict(F=PL.E.FUSED_GRAM_MAX_F + 1)),
    ("no z-score buffer", dict(side={})),
    ("z-score buffer overwritten", dict(side={"zscore": None})),
    ("collect wants the whole C", dict(collect={})),
    ("head is more than half the zoo", dict(F=63)),
    ("top needs more than 64 rows", dict(top=33)),
])
def test_not_eligible(why, kw):
    assert _head(**kw) == 0, why


def test_half_the_zoo_is_the_limit():
    assert _head(F=64) == 32 and _head(F=63) == 0
    assert _head(F=96, top=20) == 48 and _head(F=95, top=20) == 0


@pytest.mark.parametrize("top,H", [(1, 32), (5, 32), (16, 32), (17, 48), (24, 48), (25, 64), (32, 64), (33, 80)])
def test_head_rows_default(monkeypatch, top, H):
    monkeypatch.delenv("FMX_GRAM_HEAD", raising=False)
    assert PL.gram_head_size(top) == H


@pytest.mark.parametrize("env,top,H", [("16", 5, 16), ("16", 8, 16), ("16", 9, 32), ("48", 5, 48), ("64", 5, 64),
                                       ("32", 20, 48)])
def test_head_rows_env(monkeypatch, env, top, H):
    monkeypatch.setenv("FMX_GRAM_HEAD", env)
    assert PL.gram_head_size(top) == H


@pytest.mark.parametrize("env", ["0", "24", "128", "x"])
def test_head_rows_env_rejected(monkeypatch, env):
    monkeypatch.setenv("FMX_GRAM_HEAD", env)
    with pytest.raises(ValueError):
        PL.gram_head_size(5)


def test_lazy_default_follows_env(monkeypatch):
    monkeypatch.delenv("FMX_LAZY_GRAM", raising=False)
    assert PL.StepConfig().lazy_gram is True
    monkeypatch.setenv("FMX_LAZY_GRAM", "0")
    assert PL.StepConfig().lazy_gram is False
    assert PL.workload_config("c2").lazy_gram is False
    monkeypatch.setenv("FMX_LAZY_GRAM", "1")
    assert PL.StepConfig().lazy_gram is True
