#!/usr/bin/env python3
"""Drop-in for the reference's data_preproc/gene_normals.py (same flags, same files; normals from the device): see scp_amd/cli.py."""
from scp_amd.cli import gene_normals_main

if __name__ == "__main__":
    gene_normals_main()
