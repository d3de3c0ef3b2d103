"""Shared test helpers (not collected: no test_ prefix)."""
