"""Minimal M4A (MP4) writer for ALAC packets: the writer lives in the product package now (alac.net_amd.container, behind
alac.net_amd.save); this module keeps the old import working for tests and tools."""
from ..container import _atom, alac_specific_config, write_m4a  # noqa: F401
