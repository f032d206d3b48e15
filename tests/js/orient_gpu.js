'use strict';
/* Oriented feeds from the JavaScript host, on a GPU (driven by tests/test_gpu_orient.py):
 *     node tests/js/orient_gpu.js job.json
 * job: { w, h, dir, video: {file, want, width, height, format, matrix, orientation, rect | null},
 *        feeds: [{file (one packed STORED frame), want (the expected canvas, RGBA), width, height, format, matrix, orientation, rect | null}] } —
 * expectations: the oracle's resampler on the numpy-oriented declared conversion, rects in the oriented frame's coordinates.
 *  1. ccv.drawFrames of the oriented video: the canvas equals `want` byte for byte;
 *  2. ccv.DeviceBatch with opts.sources that carry `orientation`: drawList into a frame set and drawListBound — whitebalance and detectStep
 *     equal those of a second batch that got the expected canvases by upload(); ONE drawListDevice per draw.
 * Prints "orient_gpu: ok" or the failed checks. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const errors = [];
let checks = 0;
function check(cond, msg) { checks++; if (!cond && errors.length < 20) errors.push(msg); return cond; }
function same(a, b) { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false; return true; }
const read = function (name) { return new Uint8Array(fs.readFileSync(path.join(job.dir, name))); };
const n = job.feeds.length, fb = job.w * job.h * 4;

/* 1. ccv.drawFrames */
const v = job.video, canvas = new Canvas(job.w, job.h);
headtrackr.ccv.drawFrames({ width: v.width, height: v.height, format: v.format, matrix: v.matrix, orientation: v.orientation, data: read(v.file) }, canvas, v.rect);
check(same(canvas.getContext('2d').getImageData(0, 0, job.w, job.h).data, read(v.want)), 'ccv.drawFrames of the oriented video');

/* 2. DeviceBatch */
let listDraws = 0;
const realList = A.drawListDevice;
A.drawListDevice = function () { listDraws++; return realList.apply(this, arguments); };
const sources = job.feeds.map(function (f) { return { width: f.width, height: f.height, format: f.format, matrix: f.matrix, orientation: f.orientation, sets: 1 }; });
const rects = job.feeds.map(function (f) { return f.rect; });
const want = new Uint8Array(n * fb);
job.feeds.forEach(function (f, i) { want.set(read(f.want), i * fb); });
const ref = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 1 });
ref.upload(want, 0);
const refWb = ref.whitebalance(0), refBest = ref.detectStep(0).best;
const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 1, sources: sources });
job.feeds.forEach(function (f, i) { b.uploadSourceOf(i, read(f.file), 0); });
b.drawList(0, 0, rects);
check(same(b.whitebalance(0), refWb), 'whitebalance of the set drawList drew');
check(same(b.detectStep(0).best, refBest), 'detectStep on the set drawList drew');
b.drawListBound(0, rects);
check(same(b.whitebalance(-1), refWb), 'whitebalance after drawListBound');
check(listDraws === 2, 'ONE drawListDevice per draw (' + listDraws + ')');
let threw = false;
try { b.drawList(0, 0, rects.map(function (r, i) { return i === 0 ? [0, 0, job.feeds[0].width, job.feeds[0].height] : r; })); } catch (e) { threw = /status -1/.test(e.message) && /entry 0:/.test(e.message); }
check(threw, 'a rect inside the stored frame but outside the oriented one is refused with HT_ERR_INVALID, naming entry 0');
b.destroy();
ref.destroy();

process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'orient_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
