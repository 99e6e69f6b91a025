"""Mirrors of the reference's modules/transformer package.  Only `attention` is mirrored; with the reference tree importable its own
`modules.transformer` package stays the parent and `modules.transformer.model` keeps resolving to its file."""
