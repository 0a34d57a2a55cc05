"""Seeded test data shaped like one clade of MT_database: the 13 mitochondrial protein-coding genes of S species, one record per
(species, gene) with headers `gi_NC_<6 digits>_<GENE>_<Genus>_<species>_<len>_aa`.  Each gene is an ancestor protein; each species'
copy substitutes a few per cent of its residues, so peptide k-mers are shared between the records of one gene and (almost) never
between genes, as in the real database.  Gene DNA comes from oracle.prot_bait_ref.back_translate, for species in the set and for
"unseen" species mutated further from the ancestor."""
from __future__ import annotations

import random
from typing import Dict, List, Tuple

GENES = ["ATP6", "ATP8", "COX1", "COX2", "COX3", "CYTB", "ND1", "ND2", "ND3", "ND4", "ND4L", "ND5", "ND6"]
# typical lengths (residues) of the metazoan proteins
GENE_LEN = {"ATP6": 226, "ATP8": 52, "COX1": 512, "COX2": 228, "COX3": 260, "CYTB": 378, "ND1": 318, "ND2": 344, "ND3": 115,
            "ND4": 459, "ND4L": 98, "ND5": 572, "ND6": 168}
# residue frequencies of make_protein_bait (mitochondrial proteins: L, S, F, I heavy)
WEIGHTS = {"L": 16, "S": 10, "F": 9, "I": 8, "V": 7, "G": 7, "A": 6, "T": 6, "M": 5, "P": 4, "Y": 4, "N": 4,
           "W": 3, "K": 2, "E": 2, "D": 2, "H": 2, "Q": 2, "R": 2, "C": 1}
_AAS, _W = list(WEIGHTS), list(WEIGHTS.values())
GENERA = ["Mytilus", "Octopus", "Nautilus", "Haliotis", "Conus", "Aplysia", "Loligo", "Crassostrea", "Lottia", "Biomphalaria"]
EPITHETS = ["edulis", "vulgaris", "pompilius", "rubra", "textile", "californica", "bleekeri", "gigas", "gigantea", "glabrata",
            "minor", "major", "sinensis", "japonica", "borealis"]


def substitute(prot: str, rate: float, rng: random.Random) -> str:
    return "".join(rng.choices(_AAS, weights=_W)[0] if rng.random() < rate else a for a in prot)


class Clade:
    """text: the protein FASTA; records: [(name, gene, species, protein)] in file order; ancestors: gene -> protein"""

    def __init__(self, n_species: int = 10, seed: int = 20261016, sub_rate: float = 0.03, scale: float = 1.0):
        rng = random.Random(seed)
        self.rng = rng
        self.ancestors: Dict[str, str] = {g: "M" + "".join(rng.choices(_AAS, weights=_W, k=max(int(GENE_LEN[g] * scale), 30) - 1))
                                          for g in GENES}
        self.species: List[Tuple[str, str]] = []
        while len(self.species) < n_species:
            sp = (rng.choice(GENERA), rng.choice(EPITHETS) + ("" if len(self.species) < 40 else str(len(self.species))))
            if sp not in self.species:
                self.species.append(sp)
        self.records: List[Tuple[str, str, Tuple[str, str], str]] = []
        for si, sp in enumerate(self.species):
            acc = rng.randrange(10 ** 6)
            for g in GENES:
                p = substitute(self.ancestors[g], sub_rate, rng)
                self.records.append(("gi_NC_%06d_%s_%s_%s_%d_aa" % (acc, g, sp[0], sp[1], len(p)), g, sp, p))
        lines = []
        for name, _, _, p in self.records:
            lines.append(">" + name)
            lines += [p[i:i + 60] for i in range(0, len(p), 60)]
        self.text = "\n".join(lines) + "\n"

    def unseen(self, rate: float, seed: int) -> Dict[str, str]:
        """the proteins of a species that is not in the set, `rate` of the residues substituted from the ancestors"""
        rng = random.Random(seed)
        return {g: substitute(a, rate, rng) for g, a in self.ancestors.items()}


def gene_dna(proteins: Dict[str, str], code: int, seed: int) -> Dict[str, str]:
    from oracle.prot_bait_ref import back_translate
    rng = random.Random(seed)
    return {g: back_translate(p, code, rng) for g, p in proteins.items()}


def sample_reads(dna: Dict[str, str], n: int, seed: int, read_len: int = 150) -> Tuple[List[str], List[str]]:
    """n reads of read_len (or the whole gene when shorter), evenly over the genes, half of them reverse-complemented.
    -> (reads, the gene each read was sampled from)"""
    from oracle.prot_bait_ref import revcomp_any
    rng = random.Random(seed)
    genes = sorted(dna)
    seqs, truth = [], []
    for i in range(n):
        g = genes[i % len(genes)]
        s = dna[g]
        p = rng.randrange(0, max(len(s) - read_len, 0) + 1)
        r = s[p:p + read_len]
        seqs.append(revcomp_any(r) if rng.random() < 0.5 else r)
        truth.append(g)
    return seqs, truth
