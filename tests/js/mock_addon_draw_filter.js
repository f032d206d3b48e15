'use strict';
/* tests/js/mock_addon_draw_filter.js — TEST INFRASTRUCTURE: tests/js/mock_addon_draw_list.js (left as it is) plus drawListFilteredDevice and
 * drawFilterFactors of csrc/ht_napi.cc, by the rule's description: every entry is drawn by the mock's single-source draws (the declared
 * conversion and resampler) onto a FINE canvas of Nx w x Ny h, and each canvas pixel is the rounded integer mean of its Nx x Ny block.  So
 * the host logic of ccv.DeviceBatch's opts.prefilter runs without a GPU.  The borrowed draws' counters are put back: `calls` shows which
 * entry point the FACADE took.  `withDrawFilter(false)`: an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_draw_list.js'));
const DRAW_RGBA = 16;

function factor(num, den, mf) { return Math.min(mf, Math.max(1, Math.ceil(num / den))); }

const filtered = {
  drawFilterFactors: function (sizes, w, h, mf) {
    mock.calls.drawFilterFactors = (mock.calls.drawFilterFactors || 0) + 1;
    if (!(sizes instanceof Int32Array) || sizes.length % 2) throw new TypeError('mock addon: sizes is an Int32Array [2n]');
    if (!(w >= 1 && h >= 1 && mf >= 1 && mf <= 8)) throw new RangeError('mock addon: maxFactor is 1..8');
    const out = new Int32Array(sizes.length);
    for (let i = 0; i < sizes.length; i += 2) { out[i] = factor(sizes[i], w, mf); out[i + 1] = factor(sizes[i + 1], h, mf); }
    return out;
  },
  drawListFilteredDevice: function (c, entries, mf, d, dstride, doff, wait) {
    mock.calls.drawListFilteredDevice = (mock.calls.drawListFilteredDevice || 0) + 1;
    if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context');
    if (!Array.isArray(entries) || entries.length < 1 || entries.length > 65535) throw new RangeError('mock addon: 1..65535 entries');
    if (!(Number.isInteger(mf) && mf >= 1 && mf <= 8)) throw new RangeError('mock addon: maxFactor is 1..8');
    if (!(c.w > 0 && c.h > 0)) throw new Error('mock addon: status -6: no geometry');
    const n = entries.length, W = c.w, H = c.h, fb = W * H * 4, boundForm = d === null || d === undefined, ds = dstride || fb, off = doff || 0;
    if (boundForm && n > c.maxBatch) throw new Error('mock addon: status -1: entry ' + c.maxBatch + ': more entries than the batch capacity');
    const target = boundForm ? { kind: 'dev', buf: new Uint8Array(n * fb) } : d;
    if (!boundForm && off + (n - 1) * ds + fb > d.buf.length) throw new RangeError('mock addon: destination outside the device buffer');
    const saved = Object.assign({}, mock.calls);
    try {
      entries.forEach(function (e, i) {
        if (!e || !e.dev) throw new TypeError('mock addon: an entry is {dev, offset, width, height, format, matrix, rect}');
        const rect = e.rect === undefined ? null : e.rect, at = (boundForm ? 0 : off) + i * (boundForm ? fb : ds);
        const nx = factor(rect ? rect[2] : e.width, W, mf), ny = factor(rect ? rect[3] : e.height, H, mf), FW = nx * W, FH = ny * H, cnt = nx * ny;
        const fake = { kind: 'ctx', w: FW, h: FH, maxBatch: 1 }, fine = { kind: 'dev', buf: new Uint8Array(FW * FH * 4) };
        try {
          if (e.format === DRAW_RGBA) mock.drawFramesDevice(fake, e.dev, e.offset || 0, 1, e.width, e.height, 0, 0, rect, fine, 0, 0, false);
          else mock.drawFramesYuvDevice(fake, e.dev, e.offset || 0, 1, e.width, e.height, e.format, e.matrix || 0, 0, rect, fine, 0, 0, false);
        } catch (err) { err.message = 'entry ' + i + ': ' + err.message; throw err; }
        for (let y = 0; y < H; y++) for (let x = 0; x < W; x++) for (let ch = 0; ch < 4; ch++) {
          let sum = 0;
          for (let b = 0; b < ny; b++) for (let a = 0; a < nx; a++) sum += fine.buf[((ny * y + b) * FW + nx * x + a) * 4 + ch];
          target.buf[at + (y * W + x) * 4 + ch] = Math.floor((sum + (cnt >> 1)) / cnt);
        }
      });
    } finally {
      Object.keys(mock.calls).forEach(function (k) { if (k in saved) mock.calls[k] = saved[k]; else delete mock.calls[k]; });
    }
    if (boundForm) { c.frames = target.buf; c.n = n; c.stride = fb; }
    if (wait) mock.calls.drawListFilteredDeviceWaited = (mock.calls.drawListFilteredDeviceWaited || 0) + 1;
  }
};

mock.withDrawFilter = function (on) {
  Object.keys(filtered).forEach(function (k) { if (on) mock[k] = filtered[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
