"""CPU: the structure of the sharding layer.  The sharded table and the sharded index are siblings under one exchange base; the four GPU
backends take shard / shard_counts / empty from one sharding base through their own MRO, and no class borrows another class's methods."""
import inspect


def test_sharded_classes_are_siblings_under_the_exchange_base():
    from kmerhash_amd import dist as D, dist_index as X
    T, S, E = D.ShardedTable, X.ShardedKmerPositionIndex, D.ShardExchange
    assert issubclass(T, E) and issubclass(S, E) and T is not E and S is not E
    assert not issubclass(S, T) and not issubclass(T, S)
    for name in ("insert", "insert_counts", "value_histogram", "erase_values", "_query", "_late_check", "query_pieces", "_my_query_pieces"):
        assert not hasattr(S, name) and not hasattr(E, name), name
    for name in ("timings", "_span", "_single", "_host_staged", "_ctl_device", "_inject", "_status_of", "_vote", "_raise_if", "_like",
                 "_exchange_counts", "_exchange", "_offs", "_exchange_grouped", "_reduce", "_words"):
        assert name in vars(E) and name not in vars(T) and name not in vars(S), name
    assert isinstance(vars(T)["local"], property) and isinstance(vars(S)["local"], property)


def test_gpu_backends_share_one_sharding_implementation():
    from kmerhash_amd import dist as D, dist_index as X
    backends = (D.GpuBackend, D.WideGpuBackend, X.IndexGpuBackend, X.WideIndexGpuBackend)
    for name in ("shard", "shard_counts", "empty", "_permute"):
        owners = {next(c for c in b.__mro__ if name in vars(c)) for b in backends}
        assert len(owners) == 1, (name, owners)                       # one implementation, found through every backend's own MRO
        assert all(issubclass(b, next(iter(owners))) for b in backends)
    # no function in a class body was made in the body of an unrelated class
    for cls in backends + (D.ShardExchange, D.ShardedTable, X.ShardedKmerPositionIndex):
        for klass in cls.__mro__[:-1]:
            for name, v in vars(klass).items():
                f = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v.fget if isinstance(v, property) else v
                if inspect.isfunction(f):
                    assert f.__qualname__.split(".")[0] == klass.__name__, (klass.__name__, name, f.__qualname__)


def test_key_width_and_plan_attributes():
    from kmerhash_amd import dist as D, dist_index as X
    assert not hasattr(D.GpuBackend, "key_words") and hasattr(D.GpuBackend, "shard_plan")
    assert D.WideGpuBackend.key_words == 2 and not hasattr(D.WideGpuBackend, "shard_plan")
    assert not hasattr(X.IndexGpuBackend, "key_words") and not hasattr(X.IndexGpuBackend, "shard_plan")
    assert X.WideIndexGpuBackend.key_words == 2 and not hasattr(X.WideIndexGpuBackend, "shard_plan")
