"""What ``config.ReturnModel``, ``config.NoiseModel`` and ``config.EchoModel`` share -- ``of``, ``fields``, ``is_default``,
equality, hash, ``repr``, immutability and the validators' messages -- stays per class: one table over the three."""
import pytest

from lidar_transfer_amd.config import EchoModel, NoiseModel, ReturnModel

#: class, its block's key, the default ``who``, "a" / "an", a block that is on, one that is at its default, a bad number, a
#: bad integer (field, value, the message's tail)
TABLE = [
    (ReturnModel, "return_model", "return model", "a", dict(max_range=80.0, seed=3), dict(max_range=float("inf")),
     ("min_range", float("inf"), "must be finite (max_range may be +inf), not inf"),
     ("seed", 2 ** 32, "must be an integer in [0, 2^32), not 4294967296")),
    (NoiseModel, "noise_model", "noise model", "a", dict(range_sigma=0.02, seed=3), dict(range_sigma=0),
     ("range_sigma", -1, "must be finite and not negative, not -1.0"),
     ("remission_levels", 2.0, "must be an integer in [0, 2^32), not 2.0")),
    (EchoModel, "echo_model", "echo model", "an", dict(divergence=0.2, subrays=5), dict(divergence=0.2, subrays=1),
     ("ring", 0, "must be in (0, 1], not 0.0"),
     ("subrays", 9, "must be an integer in [1, 8], not 9")),
]


@pytest.mark.parametrize("cls, key, who, article, on, off, bad_number, bad_integer", TABLE, ids=[r[1] for r in TABLE])
def test_the_three_value_classes_keep_their_own_words(cls, key, who, article, on, off, bad_number, bad_integer):
    assert cls.KEY == key
    m = cls.of(on)
    assert type(m) is cls and not m.is_default and cls.of(m) is m and cls.of(None) is None
    assert list(m.fields()) == list(cls.DEFAULTS) and m.fields() == dict(cls.DEFAULTS, **on)
    assert cls.of(off) is None and cls(**off).is_default and cls.of(cls(**off)) is None and cls().is_default
    same = cls(**on)
    assert m == same and hash(m) == hash(same) and m != cls(**off) and m != on and len({m, same, cls(**off)}) == 2
    assert repr(m) == cls.__name__ + "(" + ", ".join(f"{k}={v!r}" for k, v in m.fields().items()) + ")"
    assert eval(repr(m)) == m
    with pytest.raises(AttributeError) as e:
        setattr(m, next(iter(on)), 1)
    assert str(e.value) == f"{article} {cls.__name__} does not change: make another"
    for text, make in ((f"{who}: ", lambda **kw: cls(**kw)), (f"{who}: ", lambda **kw: cls.of(kw)),
                       ("sensor 'x': ", lambda **kw: cls.of(kw, who="sensor 'x'"))):
        for name, value, tail in (bad_number, bad_integer):
            with pytest.raises(ValueError) as e:
                make(**{name: value})
            assert str(e.value) == f"{text}{key} {name} {tail}"
    name = bad_number[0]
    for value in ("1", True, None):
        with pytest.raises(ValueError) as e:
            cls(**{name: value})
        assert str(e.value) == f"{who}: {key} {name} must be a number, not {value!r}"
    with pytest.raises(ValueError) as e:
        cls.of([1, 2])
    assert str(e.value) == f"{who}: {key} must be a mapping of {', '.join(cls.DEFAULTS)}"
    with pytest.raises(ValueError) as e:
        cls.of(dict(on, zeta=1, alpha=2))
    assert str(e.value) == f"{who}: {key} has unknown key(s) alpha, zeta (known: {', '.join(cls.DEFAULTS)})"


def test_models_of_different_blocks_are_never_equal():
    r, n = ReturnModel(seed=7), NoiseModel(seed=7)
    assert r == ReturnModel(seed=7) and n == NoiseModel(seed=7)
    assert r != n and n != r and r != EchoModel() and EchoModel() != n and len({r, n, EchoModel()}) == 3
    # (nor with the very same fields: a model that was handed the other's, name by name)
    twin = NoiseModel()
    twin.__dict__.clear()
    twin.__dict__.update(r.fields())
    assert twin.__dict__ == r.__dict__ and twin != r and r != twin
    assert ReturnModel(max_range=float("inf")).is_default and ReturnModel(max_range=1e9) != ReturnModel()
    assert EchoModel(divergence=0.2).is_default and EchoModel(subrays=4).is_default     # off is EchoModel's own rule
    assert not EchoModel(divergence=0.2, subrays=2).is_default
