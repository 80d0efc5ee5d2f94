"""The contig posterior entry points at the C-ABI boundary (CPU only, no device):
cpg_contigs_posterior_d and cpg_contigs_island_confidence_d are declared, exported, bound and
reject a null context before any device call."""

NEW_SYMBOLS = ["cpg_contigs_posterior_d", "cpg_contigs_island_confidence_d"]


def test_symbols_in_signatures():
    from cpgisland_amd import _lib
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["cpg_contigs_posterior_d"]) == 12
    assert len(_lib.SIGNATURES["cpg_contigs_island_confidence_d"]) == 11


def test_symbols_exported_by_the_library():
    from cpgisland_amd import _lib
    for n in NEW_SYMBOLS:
        assert hasattr(_lib.lib, n), n


def test_python_entry_points_are_callable():
    from cpgisland_amd import device as D
    assert callable(D.contigs_posterior) and callable(D.contigs_island_confidence)


def test_null_context_is_invalid_without_a_device():
    from cpgisland_amd import _lib
    lib = _lib.lib
    assert lib.cpg_contigs_posterior_d(None, None, None, 0, None, None, None, 0, None, None,
                                       None, None) == _lib.CPG_E_INVALID
    assert b"null" in lib.cpg_last_error()
    assert lib.cpg_contigs_island_confidence_d(None, None, 0, None, None, 0, None, None, 0, None,
                                               None) == _lib.CPG_E_INVALID
    assert b"null" in lib.cpg_last_error()
